"""The block pressure solver's multigrid V-cycle and PCG on the GPU (fy_solver_precondition_host, fy_solver_solve_p_host, the coarse operators by name)
against tests/mg_ref.py, the numpy.longdouble statement of the hierarchy -- as operations, not through whole steps.  The reference is built from the
DEVICE's own level-0 coefficients, so the cycle is tested as a function of (A_0, r); the level-0 coefficients themselves are held to the CPU oracle.
tests/test_mg_reference.py holds the oracle to the same reference on the same cases (tests/mg_cases.py).

Bounds.  A coarse operator is a sum of at most a dozen products of level l - 1: 1e-13 of the level's largest diagonal.  For M^-1 r and the PCG iterates the
bound is not a constant: `e_oracle` measures how far the CPU oracle -- the same algorithm in double -- lies from the reference over the case list, which
contains the conditioning of every case, and the device gets 50 times that.  The 50 covers what the device does differently from the oracle: FMA
contraction, the order of the restriction sums, a banded Cholesky factor where the oracle inverts the coarsest operator by Gauss-Jordan, and PCG in its
single-reduction form -- each a few ulp times that conditioning.  The smallest defect that could be constructed (one level-0 coefficient off by 1e-6)
moves z by 5e-8, four orders of magnitude above.  The reported residuals are bounded through the iterate (mg_cases.residual_scale).
Measured distances: DESIGN.md, parity section."""
import numpy as np
import pytest

import mg_cases
import mg_ref

pytestmark = pytest.mark.gpu

NAMES = list(mg_cases.CASES)
_oracle, _device = {}, {}


def oracle_side(oracle, name):
    """(level-0 coefficients, distance of precondition from the reference, distance of the cut PCG iterates) of the CPU oracle, once per case"""
    if name not in _oracle:
        o = mg_cases.stepped(oracle.fv_case, oracle.FvSolver, name)
        H = mg_cases.hierarchy(o, name)
        v = mg_cases.vectors(o.Nc, float(np.abs(o.get("p_diag")).mean()))
        ez = max(mg_cases.rel(o.precondition(v[k]), H.precondition(v[k])) for k in ("random", "smooth"))
        coef = {nm: o.get(nm) for nm in ("p_diag", "p_ux", "p_uy", "p_uz")}
        o.close()
        xs, _ = mg_ref.pcg(H.apply, H.precondition, v["b"], v["x0"], max(mg_cases.CUTS))
        ex = 0.0
        for cut in mg_cases.CUTS:
            oc = mg_cases.stepped(oracle.fv_case, oracle.FvSolver, name, p_max_iter=cut)
            ex = max(ex, mg_cases.rel(oc.solve_p(v["b"], v["x0"])[0], xs[cut - 1]))
            oc.close()
        _oracle[name] = (coef, ez, ex)
    return _oracle[name]


@pytest.fixture(scope="module")
def e_oracle(oracle):
    """the largest distance of the CPU oracle from the reference over the case list: (of M^-1 r relative to max |z_ref|, of the PCG iterates relative to
    max |x_ref|).  Measured: 3.2e-14, and 5.3e-14 to 1.2e-13 (the oracle's sums follow its thread count)."""
    ez = max(oracle_side(oracle, n)[1] for n in NAMES)
    ex = max(oracle_side(oracle, n)[2] for n in NAMES)
    print(f"e_oracle: z {ez:.2e}, x {ex:.2e}")
    assert 1e-16 < ez < 1e-12 and 1e-16 < ex < 1e-12          # (the oracle's own bound, tests/test_mg_reference.py)
    return ez, ex


class Env:
    """switches for the solvers created inside the block; on the way out they are removed and one solver is created so that the library re-reads them"""

    def __init__(self, product, monkeypatch, env):
        self.product, self.mp, self.env = product, monkeypatch, env

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, v)

    def __exit__(self, *exc):
        for k in self.env:
            self.mp.delenv(k)
        if self.env:
            args, kw = mg_cases.case_kwargs("8x8x8")
            self.product.Solver(self.product.make_case(*args, **kw)).close()


def device_side(product, name):
    """everything the default-switch tests read from one stepped solver of `name`"""
    if name not in _device:
        s = mg_cases.stepped(product.make_case, product.Solver, name)
        H = mg_cases.hierarchy(s, name)
        v = mg_cases.vectors(s.n_cells, float(np.abs(s.get("p_diag")).mean()))
        levels = s.mg_levels()
        d = dict(H=H, v=v, levels=levels, coef={nm: s.get(nm) for nm in ("p_diag", "p_ux", "p_uy", "p_uz")},
                 ops=[[s.get(f"mg{l}_{a}") for a in ("diag", "ux", "uy", "uz")] for l in range(1, len(levels))],
                 z={k: s.precondition(v[k]) for k in ("random", "smooth")}, z_ref={k: H.precondition(v[k]) for k in ("random", "smooth")})
        s.close()
        _device[name] = d
    return _device[name]


def check_operators(H, ops_per_level):
    """ops_per_level[l - 1] = (diag, ux, uy, uz) of level l over the whole block"""
    worst = 0.0
    for l, ops in enumerate(ops_per_level, start=1):
        ref = H.operators(l)
        scale = float(np.abs(ref[0]).max())
        for nm, a, r in zip(("diag", "ux", "uy", "uz"), ops, ref):
            assert a.shape == r.shape, (l, nm, a.shape, r.shape)
            d = float(np.abs(np.asarray(a, np.longdouble) - r).max()) / scale
            worst = max(worst, d)
            assert d <= 1e-13, (l, nm, d)
    return worst


def check_cut_pcg(make_solver, H, v, M, bound_x, label):
    """solve_p cut at 1, 2, 3 and 6 iterations, twice on the same solver (the second solve meets the buffers the first one traded at its first iteration),
    against the reference PCG: iterate, both residuals, the count"""
    xs, res = mg_ref.pcg(H.apply, M, v["b"], v["x0"], max(mg_cases.CUTS))
    for cut in mg_cases.CUTS:
        s = make_solver(cut)
        x_scale = float(np.abs(xs[cut - 1]).max())
        rs = mg_cases.residual_scale(H, x_scale, v["b"], v["x0"])
        for run in (0, 1):
            x, it = s.solve_p(v["b"], v["x0"])
            st = s.stats()
            st = st[0] if isinstance(st, list) else st
            d = mg_cases.rel(x, xs[cut - 1])
            print(f"{label} cut {cut} run {run}: dx = {d:.2e} (bound {bound_x:.2e}), initial {st['p_initial_residual']:.15e} ref {float(res[0]):.15e}, "
                  f"final {st['p_final_residual']:.15e} ref {float(res[cut]):.15e}")
            # (one level: M^-1 = A^-1, the first iteration solves the system and a later one may meet a residual under p_tol = 1e-30)
            assert it == cut or (len(H.levels) == 1 and M == H.precondition and 1 <= it < cut and st["p_final_residual"] < 1e-30), (cut, it)
            assert d <= bound_x, (cut, run, d)
            assert abs(st["p_initial_residual"] - float(res[0])) <= bound_x * rs
            assert abs(st["p_final_residual"] - float(res[cut])) <= bound_x * rs
        s.close()


# ---- one domain ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_level0_coefficients_match_the_oracle(product, oracle, name):
    coef = oracle_side(oracle, name)[0]
    d = device_side(product, name)
    for nm in coef:
        np.testing.assert_allclose(d["coef"][nm], coef[nm], rtol=1e-9, atol=0, err_msg=nm)


@pytest.mark.parametrize("name", NAMES)
def test_hierarchy_and_coarse_operators_match_the_reference(product, name):
    d = device_side(product, name)
    assert d["levels"] == [(nx, ny, nz, False) for nx, ny, nz in d["H"].shapes]
    worst = check_operators(d["H"], d["ops"])
    print(f"{name}: coarse operators within {worst:.2e} of max |diag_l|")


@pytest.mark.parametrize("name", NAMES)
def test_precondition_matches_the_reference(product, e_oracle, name):
    d = device_side(product, name)
    for k in ("random", "smooth"):
        dist = mg_cases.rel(d["z"][k], d["z_ref"][k])
        print(f"{name} {k}: |z - z_ref| / max |z_ref| = {dist:.2e} (bound {50 * e_oracle[0]:.2e})")
        assert dist <= 50 * e_oracle[0]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("switch", ["FOAMYADE_NO_PAIRS", "FOAMYADE_NO_TAIL_CACHE"])
def test_precondition_matches_the_reference_with_a_kernel_switch(product, e_oracle, name, switch, monkeypatch):
    d = device_side(product, name)
    with Env(product, monkeypatch, {switch: "1"}):
        s = mg_cases.stepped(product.make_case, product.Solver, name)
        z = {k: s.precondition(d["v"][k]) for k in ("random", "smooth")}
        s.close()
    for k in z:
        dist = mg_cases.rel(z[k], d["z_ref"][k])
        print(f"{name} {switch} {k}: {dist:.2e}")
        assert dist <= 50 * e_oracle[0]


@pytest.mark.parametrize("name", NAMES)
def test_device_cycle_is_symmetric_and_positive(product, name):
    d = device_side(product, name)
    a, b = d["v"]["random"], d["v"]["smooth"]
    Ma, Mb = d["z"]["random"], d["z"]["smooth"]
    assert abs(Ma @ b - Mb @ a) <= 1e-12 * np.linalg.norm(Ma) * np.linalg.norm(b)
    assert Ma @ a > 0 and Mb @ b > 0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("p_solver", [1, 0])
def test_cut_pcg_matches_the_reference(product, e_oracle, name, p_solver):
    d = device_side(product, name)
    H = d["H"]
    if p_solver == 0:
        s = mg_cases.stepped(product.make_case, product.Solver, name, p_solver=0)
        assert s.mg_levels() == [H.shapes[0] + (False,)]
        H = mg_cases.hierarchy(s, name)                                     # (the same matrix: the step's other solves do not enter it)
        z = s.precondition(d["v"]["random"])
        s.close()
        assert mg_cases.rel(z, H.jacobi(d["v"]["random"])) <= 4 * np.finfo(float).eps
    check_cut_pcg(lambda cut: mg_cases.stepped(product.make_case, product.Solver, name, p_solver=p_solver, p_max_iter=cut), H, d["v"],
                  H.precondition if p_solver == 1 else H.jacobi, 50 * e_oracle[1], f"{name} p_solver {p_solver}")


@pytest.mark.parametrize("what", ["20x20x20", "12x12x12_pimple", "slabs"])
def test_hook_calls_between_steps_leave_the_run_bit_identical(product, what):
    """fluid-only steps at the default tolerances, with precondition / mg<l>_* / mg_levels calls after every step and without"""
    name = "20x20x20" if what == "slabs" else what
    args, kw = mg_cases.case_kwargs(name)
    for k in ("p_max_iter", "p_tol", "p_final_tol", "p_rel_tol"):
        kw.pop(k)
    if what == "slabs":
        args = (args[0], 16, 16, 24) + args[4:]
    n = args[1] * args[2] * args[3]
    out = []
    for hooks in (False, True):
        case = product.make_case(*args, **kw)
        s = product.VirtualSlabs(case, 2) if what == "slabs" else product.Solver(case)
        s.set("U", np.random.RandomState(3).rand(n, 3) * 0.2)
        its = []
        for step in range(4):
            s.step()
            if hooks:
                one = s.solvers[0] if what == "slabs" else s
                assert np.isfinite(s.precondition(np.random.RandomState(step).randn(n))).all()
                one.get("mg1_diag"); one.mg_levels()
                s.precondition(np.ones(n))
            st = s.stats()
            its.append((st[0] if what == "slabs" else st)["p_iters_total"])
        out.append(({nm: s.get(nm) for nm in ("U", "p", "phi_x", "phi_y", "phi_z")}, its))
        s.close()
    (a, its_a), (b, its_b) = out
    assert its_a == its_b and sum(its_a) > 0, (its_a, its_b)
    for nm in a:
        np.testing.assert_array_equal(a[nm], b[nm], err_msg=nm)


# ---- z-slabs ---------------------------------------------------------------------------------------------------------------------------------------
#         id                      dims            slabs  switches                                   distributed levels
SLABS = {
    "16x16x24_2slabs": ((16, 16, 24), 2, {}, 1),                                               # communication-avoiding cycle, level 1 replicated
    "16x16x36_3slabs": ((16, 16, 36), 3, {}, 1),
    "16x16x24_2slabs_no_deep": ((16, 16, 24), 2, {"FOAMYADE_NO_DEEP_VCYCLE": "1"}, 1),             # one exchange per sweep
    "16x16x36_3slabs_no_deep": ((16, 16, 36), 3, {"FOAMYADE_NO_DEEP_VCYCLE": "1"}, 1),
    "8x8x8_2slabs": ((8, 8, 8), 2, {}, 1),                                                     # 4 planes per slab: too thin for the deep ghost planes
    # (8 x 8 x 8 has two levels, so its level 1 cannot stay distributed; the coarse ghost plane of launch_mg_coarsen_ghost needs a distributed level 1
    # without deep ghost planes: 4 planes per slab on level 1)
    "16x16x16_2slabs_below100": ((16, 16, 16), 2, {"FOAMYADE_MG_REPLICATE_BELOW": "100"}, 2),
    "16x16x120_3slabs_below1000": ((16, 16, 120), 3, {"FOAMYADE_MG_REPLICATE_BELOW": "1000"}, 2),  # vcycle_deep on levels 0 and 1: E = 1, 2
    "16x16x80_2slabs_below1000": ((16, 16, 80), 2, {"FOAMYADE_MG_REPLICATE_BELOW": "1000"}, 2),
    "16x16x240_3slabs_below500": ((16, 16, 240), 3, {"FOAMYADE_MG_REPLICATE_BELOW": "500"}, 3),    # three distributed levels, 20 planes per slab on the last
}


def slab_solver(product, dims, n_slabs, **kw):
    args, ckw = mg_cases.case_kwargs("8x8x8", **kw)
    vs = product.VirtualSlabs(product.make_case(args[0], *dims, *args[4:], **ckw), n_slabs)
    vs.set("U", np.random.RandomState(3).rand(dims[0] * dims[1] * dims[2], 3) * 0.2)
    vs.step()
    return vs


@pytest.mark.parametrize("sid", list(SLABS))
def test_slab_cycle_and_pcg_match_the_reference(product, e_oracle, sid, monkeypatch):
    dims, n_slabs, env, depth = SLABS[sid]
    with Env(product, monkeypatch, env):
        vs = slab_solver(product, dims, n_slabs)
        H = mg_ref.Hierarchy(vs.get("p_diag"), vs.get("p_ux"), vs.get("p_uy"), vs.get("p_uz"), dims, 0)
        v = mg_cases.vectors(dims[0] * dims[1] * dims[2], float(np.abs(vs.get("p_diag")).mean()))
        # the hierarchy: the same on every rank, the distributed depth the case was chosen for, the reference's shapes
        levels = [s.mg_levels() for s in vs.solvers]
        assert all(lv == levels[0] for lv in levels)
        assert [lv[3] for lv in levels[0]] == [True] * depth + [False] * (len(H.shapes) - depth)
        assert [(nx, ny, nz * (n_slabs if dist else 1)) for nx, ny, nz, dist in levels[0]] == H.shapes
        if sid == "16x16x240_3slabs_below500":
            assert levels[0][2] == (4, 4, 20, True)
        ops = []
        for l in range(1, len(levels[0])):
            per_rank = [[s.get(f"mg{l}_{a}") for a in ("diag", "ux", "uy", "uz")] for s in vs.solvers]
            if levels[0][l][3]:
                ops.append([np.concatenate([per_rank[r][q] for r in range(n_slabs)]) for q in range(4)])
            else:
                for r in range(1, n_slabs):
                    for q in range(4):
                        np.testing.assert_array_equal(per_rank[r][q], per_rank[0][q], err_msg=f"replicated level {l} differs on rank {r}")
                ops.append(per_rank[0])
        worst = check_operators(H, ops)
        print(f"{sid}: coarse operators within {worst:.2e} of max |diag_l|")
        assert mg_cases.rel(vs.apply_p(v["random"]), H.apply(v["random"])) <= 1e-14
        for k in ("random", "smooth"):
            dist = mg_cases.rel(vs.precondition(v[k]), H.precondition(v[k]))
            print(f"{sid} {k}: |z - z_ref| / max |z_ref| = {dist:.2e} (bound {50 * e_oracle[0]:.2e})")
            assert dist <= 50 * e_oracle[0]
        vs.close()
        check_cut_pcg(lambda cut: slab_solver(product, dims, n_slabs, p_max_iter=cut), H, v, H.precondition, 50 * e_oracle[1], sid)
