"""The general-mesh pressure multigrid (csrc/ldu_amg.hip: agglomeration hierarchy, Galerkin coarse operators, V-cycle, and PCG around it) against
tests/amg_ref.py, the long-double statement, stage by stage on the cases of tests/amg_cases.py: the hierarchy and every level's aggregates and pattern
exactly; every level's coefficients and diagonal, the last level's dense inverse, M^-1 r and PCG cut after k iterations to ten times what double
arithmetic alone costs the reference (amg_cases.D64).  The level-0 matrix is the one a step of the solver left."""
import os

import numpy as np
import pytest

import amg_cases as ac
import amg_ref as ar

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ac.CASES]
BOUND = {k: ac.BOUND_FACTOR * v for k, v in ac.D64.items()}


def make_solver(product, case, **kw):
    """the case's flow with the multigrid preconditioner; FOAMYADE_AMG_PASSES is read when the solver is created"""
    a = case.solver_args()
    ctl = dict(p_solver=product.FY_PSOLVER_PCG_MG, n_non_orth=1, p_tol=1e-9, p_rel_tol=0.0, p_final_tol=1e-9, u_tol=1e-9, p_max_iter=200)
    ctl.update(kw)
    if case.ref is not None:
        ctl["p_ref_cell"] = case.ref
    if case.passes != 3:
        os.environ["FOAMYADE_AMG_PASSES"] = str(case.passes)
    try:
        s = product.LduSolver(case.mesh, 0.01, 0.01, a["u_bc"], a["u_val"], a["p_bc"], a["p_val"], **ctl)
    finally:
        os.environ.pop("FOAMYADE_AMG_PASSES", None)
    s.set("U", np.random.RandomState(3).rand(case.mesh["n_cells"], 3) * 0.05)
    return s


def reference(case, s, H=None):
    """the reference on the matrix the solver holds now (a hierarchy already built keeps its aggregates and takes the new matrix)"""
    ni = len(ar.internal_faces(case.mesh)[0])
    coef, diag = s.get("p_coef")[:ni], s.get("p_diag")
    if H is None:
        return ar.Hierarchy(case.mesh, s.geometry("magSf")[:ni], coef, diag, case.ref, case.passes)
    H.set_matrix(coef, diag)
    return H


@pytest.fixture(scope="module")
def stepped(product):
    """{case: (solver after one step, reference)}: built once, read by several tests, never stepped again"""
    made = {}

    def get(name):
        if name not in made:
            c = ac.BY_NAME[name]
            s = make_solver(product, c)
            s.step()
            made[name] = (s, reference(c, s))
        return made[name]
    yield get
    for s, _ in made.values():
        s.close()


def check_levels(s, H, what=""):
    """levels, aggregates, pattern and padding exactly; values to BOUND.  Returns {family: worst distance}"""
    assert s.mg_levels() == H.mg_levels(), what
    worst = {"coef": 0.0, "diag": 0.0}
    for l, L in enumerate(H.levels):
        nb, cf = L.ell()
        if L.agg is None:
            assert s.mg_level(l, "agg").size == 0
        else:
            assert np.array_equal(s.mg_level(l, "agg"), L.agg), (what, l)
        d_nb, d_cf, d_dg = s.mg_level(l, "nbr"), s.mg_level(l, "coef"), s.mg_level(l, "diag")
        assert np.array_equal(d_nb, nb), (what, l)
        pad = nb == np.arange(L.n)[None, :]
        assert np.all(d_cf[pad] == 0.0), (what, l)
        if l == 0:                                  # copies of the solver's own arrays
            assert np.array_equal(d_cf, cf.astype(np.float64)) and np.array_equal(d_dg, s.get("p_diag"))
            continue
        worst["coef"] = max(worst["coef"], ac.rel(d_cf, cf)); worst["diag"] = max(worst["diag"], ac.rel(d_dg, L.diag))
    last = len(H.levels) - 1
    worst["inv"] = ac.rel(s.mg_level(last, "inv"), H.coarse_inv)
    assert s.mg_level(0, "inv").size == 0 or last == 0
    print(f"{what}: " + ", ".join(f"{k} {v:.2e} (bound {BOUND[k]:.1e})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BOUND[k], (what, k, v, BOUND[k])
    return worst


def check_cycle(s, H, case, what=""):
    worst = {}
    for nm, r in ac.probe_vectors(H, s.geometry("C"), case.ref).items():
        worst[nm] = ac.rel(s.apply("p_precondition", r), H.precondition(r))
    print(f"{what}: M^-1 r " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bound {BOUND['cycle']:.1e})")
    for nm, v in worst.items():
        assert v <= BOUND["cycle"], (what, nm, v, BOUND["cycle"])


@pytest.mark.parametrize("name", NAMES)
def test_hierarchy_and_coarse_operators_match_the_reference(stepped, name):
    s, H = stepped(name)
    c = ac.BY_NAME[name]
    assert s.mg_levels() == c.levels
    # the matrix the solver applies is the one the reference was handed
    r = np.random.RandomState(1).standard_normal(H.levels[0].n)
    assert ac.rel(s.apply("p_matrix", r), H.apply(r)) <= 1e-14
    check_levels(s, H, name)


@pytest.mark.parametrize("name", NAMES)
def test_the_cycle_matches_the_reference(stepped, name):
    s, H = stepped(name)
    check_cycle(s, H, ac.BY_NAME[name], name)


def test_the_tail_cap_binds_with_one_pass_on_the_sheared_block(stepped):
    """six levels, five of them of at most 1024 cells: only four go into the one-workgroup tail, level 1 (797 cells) is launched sweep by sweep"""
    s, H = stepped("sheared_1pass")
    assert len(s.mg_levels()) == 6 and [n for n, _ in s.mg_levels()][1:] == [797, 369, 172, 81, 39]
    assert int(H.levels[0].agg[ac.BY_NAME["sheared_1pass"].ref]) != 0


def test_single_level_cycle_inverts_the_matrix(stepped):
    s, H = stepped("single_level")
    assert s.mg_levels() == [(64, 6)]
    rs = np.random.RandomState(4)
    for x in (rs.standard_normal(64), np.ones(64), np.eye(1, 64, 0).ravel()):
        back = s.apply("p_precondition", s.apply("p_matrix", x))
        assert ac.rel(back, x) <= BOUND["cycle"], ac.rel(back, x)


@pytest.mark.parametrize("cut", ac.PCG_CUTS)
@pytest.mark.parametrize("name", ["small_renumbered", "odd_block_1pass", "through_flow", "sheared_1pass", "two_launched_levels", "cyclic"])
def test_cut_pcg_matches_the_reference(product, name, cut):
    """one corrector, no non-orthogonal pass, tolerances 0 and p_max_iter = k: the step's one pressure solve is k iterations from the p it started with
    on the p_rhs it leaves behind -- against long-double PCG preconditioned with the reference cycle.  The second step, so that the first guess is no
    zero field"""
    c = ac.BY_NAME[name]
    s = make_solver(product, c, n_correctors=1, n_non_orth=0, p_tol=0.0, p_rel_tol=0.0, p_final_tol=0.0, p_final_rel_tol=0.0, p_max_iter=cut)
    s.step()
    p0 = s.get("p")
    s.step()
    assert s.stats()["p_iters_total"] == cut
    H = reference(c, s)
    xs, res = ar.pcg(H.apply, H.precondition, s.get("p_rhs"), p0, cut)
    d = ac.rel(s.get("p"), xs[-1])
    print(f"{name} k={cut}: {d:.2e} (bound {BOUND['pcg']:.1e}); residual {float(res[0]):.2e} -> {float(res[-1]):.2e}")
    assert np.abs(p0).max() > 0 and float(res[-1]) < float(res[0])
    assert d <= BOUND["pcg"], (d, BOUND["pcg"])
    s.close()


@pytest.mark.parametrize("name,non_orth", [("small_renumbered_1pass", 0), ("odd_block", 2), ("two_launched_levels", 1), ("single_level", 2)])
def test_a_second_step_renews_every_level(product, name, non_orth):
    """new coefficients, same hierarchy: the coarse operators, the last level's inverse and the cycle follow the new matrix -- with non-orthogonal
    correctors too, whose passes renew only the right-hand side"""
    c = ac.BY_NAME[name]
    s = make_solver(product, c, n_non_orth=non_orth)
    s.step()
    H = reference(c, s)
    first = (H.levels[0].coef.copy(), H.coarse_inv.copy())
    s.step()
    H = reference(c, s, H)
    assert ac.rel(H.levels[0].coef, first[0]) > 1e-6 and ac.rel(H.coarse_inv, first[1]) > 1e-6      # the matrix did change
    check_levels(s, H, f"{name} step 2")
    check_cycle(s, H, c, f"{name} step 2")
    s.close()


@pytest.mark.parametrize("name", ["small_renumbered", "sheared_1pass"])
def test_runs_repeat_and_read_outs_leave_them_bit_identical(product, name):
    """three steps, three times: twice plainly, once with every read-out and both operators called after every step"""
    c = ac.BY_NAME[name]
    out = []
    for hooks in (False, False, True):
        s = make_solver(product, c, p_tol=1e-6, p_final_tol=1e-6, u_tol=1e-6)
        its = []
        for step in range(3):
            s.step()
            its.append(s.stats()["p_iters_total"])
            if hooks:
                for l in range(len(s.mg_levels())):
                    for a in ("diag", "coef", "nbr", "agg", "inv"):
                        s.mg_level(l, a)
                r = np.random.RandomState(step).standard_normal(c.mesh["n_cells"])
                assert np.isfinite(s.apply("p_precondition", r)).all() and np.isfinite(s.apply("p_matrix", r)).all()
        out.append(({nm: s.get(nm) for nm in ("U", "p", "phi")}, its))
        s.close()
    assert sum(out[0][1]) > 0
    for other in out[1:]:
        assert other[1] == out[0][1]
        for nm in out[0][0]:
            np.testing.assert_array_equal(other[0][nm], out[0][0][nm], err_msg=nm)


def test_a_level_that_is_not_there_is_an_error(product, stepped):
    s, _ = stepped("small_renumbered")
    with pytest.raises(product.FoamYadeError):
        s.mg_level(2, "diag")
    with pytest.raises(product.FoamYadeError):
        s.mg_level(0, "lower")
