"""The solid-phase statistics (fy_solver_set_solid_statistics, fy_ldu_solver_set_solid_statistics) on the device against tests/solid_stats_ref.py -- the numpy
restatement written from the definitions, itself held to its known answers in tests/test_solid_stats_ref.py.

The bar on the eight sums is derived, not chosen: a sum of m terms in any order, each term formed by at most three roundings, differs from the exact sum by at most
(m + 3) 2^-53 sum |term|; m and sum |term| are formed per cell from the stencils, and twice that is allowed between device and numpy, both being rounded.  The
fields follow from the sums by a specified operation order, so they are compared bit for bit with the restatement's formulae applied to the device's own sums."""
import numpy as np
import pytest

import field_average_ref as far
import poly_meshes as pm
import solid_stats_ref as ssr
from test_heat_transfer import WATER, assert_field, cloud, one_per_cell, thermal
from test_ldu_heat import containing_cells

pytestmark = pytest.mark.gpu

FIELDS = ("nParticle", "solidFraction", "uSolid", "granularTemperature", "dSauter")
NAMES = ("solidMoments",) + FIELDS + ("TParticle",)
BOX = 0.1


def sizes(n, ratio, mean=0.01):
    h = ratio ** (np.arange(n) / (n - 1.0))
    return h * (mean * n / h.sum())


class Rig:
    """a solver with the statistics on, its cell count, its cell volumes as the library holds them and the box its particles go into"""

    def __init__(self, product, kind, th=None, stats=1, solver=1):
        self.kind, self.block = kind, kind in ("u8", "u16", "graded")
        kw = dict(solid_stats=stats)
        if th is not None:
            kw["thermal"] = th
        if self.block:
            n = {"u8": (8, 8, 8), "u16": (16, 16, 16), "graded": (8, 6, 10)}[kind]
            dx = 0.1 / 8 if solver == 0 else 0.01
            if kind == "graded":
                h = [sizes(n[0], 2.0), sizes(n[1], 0.6), sizes(n[2], 1.5)]
                kw["grading"] = tuple(h)
                self.V = ((h[0][None, None, :] * h[1][None, :, None]) * h[2][:, None, None]).ravel()
                self.hi = np.array([a.sum() for a in h])
            else:
                self.V = np.full(n[0] * n[1] * n[2], (dx * dx) * dx)
                self.hi = np.array(n) * dx
            self.n, self.dx = n, dx
            if solver == 1:
                case = product.make_case(1, *n, dx, 2e-4, 1e-5, g=(0, 0, -9.81), p_bc=[2] * 6, **kw)
            else:
                u_val = [(0, 0, 0)] * 6
                u_val[3] = (1.0, 0, 0)
                case = product.make_case(0, *n, dx, 1e-3, 1e-2, u_val=u_val, **kw)
            self.s = product.Solver(case)
            self.Nc = n[0] * n[1] * n[2]
        else:
            if kind == "wavy_hex":
                self.mesh = pm.hex_block(7, 7, 7, (BOX, BOX, BOX), pm.wavy(0.2 * BOX / 7, (BOX, BOX, BOX)), renumber_seed=8)
            else:
                self.mesh = pm.prism_block(5, 5, 6, (BOX, BOX, BOX), pm.wavy(0.15 * BOX / 5, (BOX, BOX, BOX)))
            u_val = [(0, 0, 0)] * 6
            if solver == 1:
                self.s = product.LduSolver(self.mesh, 2e-4, 1e-5, [0] * 6, u_val, [2] * 6, solver=1, g=(0, 0, -9.81), n_non_orth=1, p_max_iter=5000, **kw)
            else:
                u_val[3] = (1.0, 0, 0)
                self.s = product.LduSolver(self.mesh, 1e-3, 1e-2, [0] * 6, u_val, [0] * 6, **kw)
            self.Nc = self.mesh["n_cells"]
            self.V = self.s.get("V")
            self.hi = np.array([BOX, BOX, BOX])
        self.s.hold_sources(True)

    def cloud(self, n, seed, outside=0, radius=0.002, speed=0.3, fill=0.7):
        return cloud(n, 0.04 * self.hi, np.array([0.96, 0.96, fill]) * self.hi, radius, seed, speed=speed, outside=outside)

    def point_cells(self, rec):
        """the containing cell of every record (-1: outside), worked out on the CPU"""
        if self.block:
            n, dx = self.n, self.dx
            inside = ((rec[:, 0:3] >= 0) & (rec[:, 0:3] <= self.hi)).all(axis=1)
            ijk = np.minimum(np.floor(rec[:, 0:3] / dx).astype(int), np.array(n) - 1)
            return np.where(inside, ijk @ np.array([1, n[0], n[0] * n[1]]), -1)
        return containing_cells(self.s, self.mesh, rec[:, 0:3])

    def reference(self, batches, Tps=None, point=False):
        items = []
        for bi, b in enumerate(batches):
            if point:
                k, ids, w = ssr.point_stencils(self.point_cells(b))
            else:
                k, ids, w, chain = self.s.stencils_of(bi)
            items.append((b, k, ids, w, None if Tps is None else Tps[bi]))
        return ssr.moments(items, self.Nc), items

    def check_sums(self, batches, what, Tps=None, point=False):
        (S, m, A), items = self.reference(batches, Tps, point)
        dev = self.s.get("solidMoments").reshape(self.Nc, 8)
        err, bound = np.abs(dev - S), 2.0 * ssr.sum_bound(m, A)
        worst = (err / np.where(bound > 0, bound, 1.0)).max(axis=0)
        print(f"{what}: cells touched {int((m > 0).sum())} of {self.Nc}, most terms in a cell {int(m.max())}; |device - numpy| / bound per sum: " + " ".join(f"{x:.2f}" for x in worst))
        assert (err <= bound).all(), (what, worst)
        assert (dev[m == 0] == 0.0).all()
        return dev, S, m, A, items

    def check_fields(self, dev, thermal_on=False):
        ref = ssr.fields(dev, self.V, thermal_on)
        for nm, x in ref.items():
            np.testing.assert_array_equal(self.s.get(nm).reshape(x.shape), x, err_msg=nm)
        return ref

    def close(self):
        self.s.close()


GAUSSIAN = ["u8", "u16", "graded", "wavy_hex", "prisms"]
NPART = {"u8": 600, "u16": 2000, "graded": 700, "wavy_hex": 500, "prisms": 500}


# ---- 1. the raw sums, after step 1 and after step 2; 2. the fields from the device's own sums ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GAUSSIAN)
def test_gaussian_sums_match_the_restatement(product, kind):
    r = Rig(product, kind)
    rec = r.cloud(NPART[kind], 5, outside=NPART[kind] // 20)
    rec[:, 9] *= 0.6 + 0.8 * np.random.RandomState(6).random_sample(rec.shape[0])
    rs = np.random.RandomState(7)
    assert np.abs(r.s.get("solidMoments")).max() == 0.0 and np.abs(r.s.get("uSolid")).max() == 0.0      # zero before the first coupling call
    for step in (1, 2):
        rec[:, 0:3] += 1e-4 * rs.standard_normal((rec.shape[0], 3))
        r.s.set_particles(rec)
        r.s.step()
        dev, S, m, A, items = r.check_sums([rec], f"{kind} step {step}")
        assert (m > 0).sum() > 50 and m.max() >= 3
    f = r.check_fields(dev)
    assert f["granularTemperature"].max() > 0 and f["dSauter"].max() > 0 and f["solidFraction"].max() > 0
    r.close()


@pytest.mark.parametrize("kind", ["u8", "prisms"])
def test_point_mode_sums_match_the_restatement(product, kind):
    r = Rig(product, kind, solver=0)
    rec = cloud(600, (0.0, 0.0, 0.0), r.hi, 0.05 * 0.0125, 43, speed=0.2, outside=20)
    rec[:, 9] *= 0.6 + 0.8 * np.random.RandomState(8).random_sample(600)
    for step in (1, 2):
        r.s.set_particles(rec)
        r.s.step()
        dev, S, m, A, items = r.check_sums([rec], f"point {kind} step {step}", point=True)
        cell = r.point_cells(rec)
        assert (r.s.found() == np.where(cell >= 0, 1, -1)).all() and (cell[:20] == -1).all() and m.max() >= 3
    r.check_fields(dev)
    assert abs(dev[:, 0].sum() - (cell >= 0).sum()) == 0.0      # w = 1: whole numbers, exact
    r.close()


# ---- 3. more distinct cells than the workgroup's table holds ----------------------------------------------------------------------------------------------------------
def test_table_overflow_drops_nothing(product):
    """512 particles -- one workgroup -- spread over the whole 16^3 block: their stencils name more than the 1 024 cells the LDS table has slots for, so part of the
    scatter leaves the kernel as direct atomics from the particle's lane beside the flush of the full table"""
    r = Rig(product, "u16")
    rec = r.cloud(512, 31, fill=0.96)
    for step in (1, 2):
        r.s.set_particles(rec)
        r.s.step()
        k, ids, w, chain = r.s.stencils_of(0)
        reach = np.unique(ids[(ids >= 0) & (k > 0)[:, None]]).size
        print(f"distinct cells of the workgroup: {reach} (table: 1024 slots)")
        assert reach > 1024
        dev, S, m, A, items = r.check_sums([rec], f"overflow step {step}")
    r.check_fields(dev)
    r.close()


# ---- 4. all batches are summed; a batch may change its size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "wavy_hex"])
def test_batches_are_summed_and_may_change_size(product, kind):
    r = Rig(product, kind)
    rec = r.cloud(1500, 9)
    for step, cut in ((1, 900), (2, 600), (3, 600)):
        batches = [rec[:cut], rec[cut:]]
        r.s.set_particle_batches(batches)
        r.s.step()
        dev, S, m, A, items = r.check_sums(batches, f"{kind} two batches, step {step}")
        shared = np.intersect1d(items[0][2][items[0][2] >= 0], items[1][2][items[1][2] >= 0]).size
        assert shared > 50
        # what one batch alone would give is less: the second batch's terms are in
        S0 = ssr.moments(items[:1], r.Nc)[0]
        assert (dev[:, 0] > S0[:, 0] + 0.5 * (S[:, 0] - S0[:, 0]))[S[:, 0] - S0[:, 0] > 1e-6].all()
    r.check_fields(dev)
    r.close()


# ---- 5. particles outside the mesh and particles nobody located -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["graded", "prisms"])
def test_unlocated_particles_contribute_nothing(product, kind):
    r = Rig(product, kind)
    rec = r.cloud(800, 13, outside=120)
    r.s.set_particles(rec)
    r.s.step()
    dev, S, m, A, items = r.check_sums([rec], f"{kind} with 120 outside")
    k = items[0][1]
    assert (k[:120] == 0).all() and (k[120:] > 0).mean() > 0.9
    d = 2.0 * rec[k > 0, 9]
    vp = np.pi * d ** 3 / 6.0
    pairs = m.sum()
    print(f"sum s0 = {dev[:, 0].sum():.15g} for {int((k > 0).sum())} located particles; sum s1 = {dev[:, 1].sum():.15e}, sum Vp = {vp.sum():.15e}")
    # sum_c w = 1 to the normalisation's rounding (k + 1 roundings per particle), then `pairs` terms summed
    assert abs(dev[:, 0].sum() - (k > 0).sum()) <= 2.0 * (pairs + 20.0) * ssr.U53 * (k > 0).sum()
    assert abs(dev[:, 1].sum() - vp.sum()) <= 2.0 * (pairs + 20.0) * ssr.U53 * vp.sum()
    r.close()


# ---- 6. the known answers ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "wavy_hex"])
def test_known_answers_on_the_device(product, kind):
    r = Rig(product, kind)
    # every particle the same velocity and the same radius
    v, rad = np.array([0.3, -1.7, 0.9]), 0.0017
    rec = r.cloud(500, 17, radius=rad)
    rec[:, 3:6] = v
    r.s.set_particles(rec)
    r.s.step()
    dev, S, m, A, items = r.check_sums([rec], f"{kind} uniform velocity")
    gT, d32, uS = r.s.get("granularTemperature"), r.s.get("dSauter"), r.s.get("uSolid").reshape(-1, 3)
    bound = ssr.theta_bound(dev, m, np.abs(dev))
    print(f"uniform velocity: granularTemperature max {gT.max():.3e} (|v|^2 / 3 = {(v * v).sum() / 3:.3e}), bound max {bound.max():.3e}")
    assert (gT <= bound).all() and (gT >= 0).all()
    assert (np.abs(uS - v)[m > 0] <= (2.0 * (m[m > 0, None] + 3.0) + 2.0) * ssr.U53 * np.abs(v)).all()
    d = 2.0 * rad
    # s1 / s6 = (pi d^3 / 6) sum w / (d^2 sum w): the two sums carry bound 1 each; Vp, d^2 and the formula add ten roundings
    assert (np.abs(d32 - d)[m > 0] <= (2.0 * (m[m > 0] + 3.0) + 10.0) * ssr.U53 * d).all() and (d32[m == 0] == 0).all()
    # pairs of identical particles at one position with velocities +-u
    u = np.array([0.4, -0.25, 1.1])
    a = r.cloud(300, 19)
    a[:, 3:6] = u
    b = a.copy()
    b[:, 3:6] = -u
    both = np.concatenate([a, b])
    r.s.set_particles(both)
    r.s.step()
    dev, S, m, A, items = r.check_sums([both], f"{kind} +-u pairs")
    k, ids, w = items[0][1], items[0][2], items[0][3]
    np.testing.assert_array_equal(ids[:300], ids[300:]); np.testing.assert_array_equal(w[:300], w[300:])
    gT, uS = r.s.get("granularTemperature"), r.s.get("uSolid").reshape(-1, 3)
    t = m > 0
    s1 = dev[t, 1]
    assert (np.abs(uS[t]) <= (ssr.sum_bound(m, A)[t, 2:5] / s1[:, None]) * (1.0 + 1e-12)).all()
    u2 = (u * u).sum()
    print(f"+-u pairs: max |granularTemperature - |u|^2 / 3| = {np.abs(gT[t] - u2 / 3).max():.3e}, max |uSolid| = {np.abs(uS).max():.3e}")
    assert (np.abs(gT[t] - u2 / 3.0) <= ssr.theta_bound(dev, m, A)[t] + 4 * ssr.U53 * u2).all() and (gT[~t] == 0).all()
    r.close()


# ---- 7. heat transfer on: TParticle ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own", [False, True], ids=["callers_Tp", "library_Tp"])
@pytest.mark.parametrize("kind", ["u8", "wavy_hex"])
def test_TParticle_weighs_the_end_of_step_temperatures(product, kind, own):
    th = thermal(product, 100, T_initial=300.0, particle_temperature=340.0, particle_cp=0.05 if own else 0.0, **WATER)
    r = Rig(product, kind, th=th)
    rec = r.cloud(600, 23, outside=10)
    rs = np.random.RandomState(24)
    Tp0 = 280.0 + 90.0 * rs.random_sample(600)
    r.s.set_particles(rec)
    r.s.set_particle_temperatures(Tp0)
    for step in (1, 2):
        r.s.set_particles(rec)
        if not own:
            r.s.set_particle_temperatures(Tp0)
        r.s.step()
        Tp = r.s.particle_temperatures()
        dev, S, m, A, items = r.check_sums([rec], f"{kind} thermal step {step}", Tps=[Tp])
    if own:
        assert np.abs(Tp - Tp0)[items[0][1] > 0].min() > 0           # the library moved them: the sums weigh the new ones
    else:
        np.testing.assert_array_equal(Tp, Tp0)
    f = r.check_fields(dev, thermal_on=True)
    t = m > 0
    assert f["TParticle"][t].min() >= Tp.min() * (1 - 1e-12) and f["TParticle"][t].max() <= Tp.max() * (1 + 1e-12) and np.ptp(f["TParticle"][t]) > 1.0
    # a batch without an array of its own: the uniform value
    if not own:
        r.s.set_particles(rec)
        r.s.set_particle_temperatures(None)
        r.s.step()
        r.check_sums([rec], f"{kind} uniform Tp", Tps=[340.0])
    r.close()


def test_without_heat_transfer_there_is_no_TParticle(product):
    for kind in ("u8", "prisms"):
        r = Rig(product, kind)
        r.s.set_particles(r.cloud(300, 3))
        r.s.step()
        with pytest.raises(product.FoamYadeError) as e:
            r.s.get("TParticle")
        assert "TParticle" in str(e.value)
        M = r.s.get("solidMoments").reshape(-1, 8)
        assert (M[:, 7] == 0.0).all() and M[:, 1].max() > 0
        r.close()


# ---- 8. off means off -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "wavy_hex"])
def test_off_launches_nothing_and_knows_no_name(product, kind):
    r = Rig(product, kind, stats=0)
    r.s.enable_kernel_timing(True)
    rec = r.cloud(300, 3)

    def refused():
        for nm in NAMES:
            with pytest.raises(product.FoamYadeError) as e:
                r.s._size(nm)
            assert nm in str(e.value) and "unknown" in str(e.value)
    for _ in range(3):
        r.s.set_particles(rec)
        r.s.step()
    assert r.s.kernel_timing("solid_stats") == (0.0, 0)
    refused()
    with pytest.raises(product.FoamYadeError):
        r.s.set_field_average([("granularTemperature", False)])
    r.s.set_solid_statistics(True)
    assert np.abs(r.s.get("solidMoments")).max() == 0.0
    r.s.set_particles(rec)
    r.s.step()
    ms, launches = r.s.kernel_timing("solid_stats")
    assert launches == 1 and ms > 0 and r.s.get("solidFraction").max() > 0
    r.check_sums([rec], f"{kind} switched on")
    r.s.set_solid_statistics(False)
    refused()
    r.s.set_particles(rec)
    r.s.step()
    assert r.s.kernel_timing("solid_stats")[1] == 1
    r.close()


# ---- 9. on changes nothing else ------------------------------------------------------------------------------------------------------------------------------------
def test_ico_cavity_is_bitwise_unchanged_by_the_statistics(product):
    n, dx = 8, 0.1 / 8
    rec = one_per_cell(n, n, n, dx, 200, 11)
    out = []
    for on in (0, 1):
        r = Rig(product, "u8", stats=on, solver=0)
        for _ in range(3):
            r.s.set_particles(rec)
            r.s.step()
        out.append((r.s.get("U"), r.s.get("p"), r.s.get("uSource"), r.s.forces(), r.s.found()))
        if on:
            assert r.s.get("nParticle").max() > 0
        r.close()
    for a, b, nm in zip(out[0], out[1], ("U", "p", "uSource", "forces", "found")):
        np.testing.assert_array_equal(a, b, err_msg=nm)
    assert (out[0][4] == 1).all() and np.abs(out[0][3]).max() > 0 and np.abs(out[0][2]).max() > 0


def test_pimple_box_is_unchanged_by_the_statistics(product):
    out = []
    for on in (0, 1):
        r = Rig(product, "u16", stats=on)
        rec = r.cloud(2000, 3)
        for _ in range(3):
            r.s.set_particles(rec)
            r.s.step()
        out.append((r.s.get("U"), r.s.get("p"), r.s.get("uSource"), r.s.get("alpha"), r.s.forces()))
        r.close()
    for a, b, nm in zip(out[0], out[1], ("U", "p", "uSource", "alpha", "forces")):
        assert_field(b, a, nm, scale=np.abs(a).max())        # (the Gaussian scatters add through atomics: two runs of the same code differ in the last bits)
    assert np.abs(out[0][0]).max() > 0 and out[0][3].min() < 1.0


# ---- 10. fieldAverage and the monitors take the fields -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "prisms"])
def test_field_average_and_monitors_take_the_fields(product, kind):
    r = Rig(product, kind)
    r.s.set_field_average([("granularTemperature", True), ("uSolid", True)])
    r.s.set_monitors([dict(name="solids", kind="vol", operation="volIntegrate", fields=["solidFraction"])])
    gT, uS = far.Item((r.Nc,), True, "time"), far.Item((r.Nc, 3), True, "time")
    rec = r.cloud(500, 9)
    rs = np.random.RandomState(10)
    s1 = []
    for step in range(5):
        rec[:, 0:3] += 2e-4 * rs.standard_normal((500, 3))
        rec[:, 3:6] = 0.3 * rs.standard_normal((500, 3))
        r.s.set_particles(rec)
        r.s.step()
        dt = r.s.stats()["delta_t"]
        gT.add(r.s.get("granularTemperature"), dt); uS.add(r.s.get("uSolid"), dt)
        s1.append(r.s.get("solidMoments").reshape(-1, 8)[:, 1])
    np.testing.assert_array_equal(r.s.get("granularTemperatureMean"), gT.m)
    np.testing.assert_array_equal(r.s.get("granularTemperaturePrime2Mean"), gT.P)
    np.testing.assert_array_equal(r.s.get("uSolidMean").reshape(-1, 3), uS.m)
    np.testing.assert_array_equal(r.s.get("uSolidPrime2Mean").reshape(-1, 6), uS.P)
    assert gT.m.max() > 0 and gT.P.max() > 0
    assert r.s.monitor_layout(0) == ["volIntegrate(solidFraction)"]
    t, rows = r.s.monitor_rows(0)
    assert rows.shape == (5, 1)
    for step in range(5):
        # sum_c (s1 / V) V: Nc terms of two roundings each, against numpy's sum of the same s1
        tot = s1[step].sum()
        print(f"step {step}: volIntegrate(solidFraction) = {rows[step, 0]:.15e}, sum s1 = {tot:.15e}")
        assert abs(rows[step, 0] - tot) <= 2.0 * (r.Nc + 3.0) * ssr.U53 * tot and tot > 0
    r.close()


# ---- 11. refusals by name ---------------------------------------------------------------------------------------------------------------------------------------------
def test_slabs_refuse_the_statistics_by_name(product):
    case = product.make_case(1, 8, 8, 20, 0.01, 2e-4, 1e-5, p_bc=[2] * 6, solid_stats=1)
    with pytest.raises(product.FoamYadeError) as e:
        product.VirtualSlabs(case, 2)
    assert "error 5" in str(e.value) and "slab" in str(e.value) and "solid statistics" in str(e.value)


@pytest.mark.parametrize("kind", ["u8", "wavy_hex"])
def test_fibre_coupling_and_writes_are_refused(product, kind):
    r = Rig(product, kind)
    rec = r.cloud(200, 7)
    r.s.set_particles(rec)
    r.s.step()
    before = r.s.get("solidMoments"), r.s.get("U")
    for nm in NAMES[:-1]:
        with pytest.raises(product.FoamYadeError) as e:
            r.s.set(nm, np.zeros(r.s._size(nm)))
        assert "error 1" in str(e.value) and nm in str(e.value)
    product._check(product.lib().fy_set_fibre_coupling(r.s._cpl, 1))
    with pytest.raises(product.FoamYadeError) as e:
        r.s.step()
    assert "error 5" in str(e.value) and "fibre" in str(e.value) and "solid statistics" in str(e.value)
    np.testing.assert_array_equal(r.s.get("solidMoments"), before[0])      # nothing was scattered, nothing solved
    np.testing.assert_array_equal(r.s.get("U"), before[1])
    product._check(product.lib().fy_set_fibre_coupling(r.s._cpl, 0))
    r.s.set_particles(rec)
    r.s.step()
    r.close()
