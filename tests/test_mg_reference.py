"""The CPU oracle's multigrid V-cycle and PCG (oracle/fv_oracle.cpp) against tests/mg_ref.py, a numpy.longdouble statement of the same hierarchy that is
rebuilt from the level-0 coefficients alone: with this file the oracle's multigrid is no longer its own witness.  tests/test_mg_parity.py holds the HIP
solver to the same reference on the same cases (tests/mg_cases.py).

Bounds.  The oracle computes in double what the reference computes in long double, so their distance is the oracle's rounding: eps = 1.1e-16 times the
operations a value passes through (about a hundred per level, up to seven levels) and the conditioning of the coarsest operator, whose exact solve
amplifies the error of its right-hand side -- with the reference cell's point term as its smallest eigenvalue that is 1e2 to 1e3 here.  1e-12 of the
result's largest entry leaves a margin over that product (measured: 5e-16 to 3.3e-14) and stays four orders of magnitude under the smallest defect that
could be constructed (one level-0 coefficient off by 1e-6: 5e-8), and eleven under a missing reference-cell term.  The residuals are bounded through the
iterate: they move by at most sum |A| |dx| / normFactor (mg_cases.residual_scale)."""
import numpy as np
import pytest

import mg_cases
import mg_ref

TOL = 1e-12
_cache = {}


def setup(oracle, name):
    """oracle solver after its one step, reference hierarchy from the oracle's level-0 coefficients, the shared vectors"""
    if name not in _cache:
        o = mg_cases.stepped(oracle.fv_case, oracle.FvSolver, name)
        H = mg_cases.hierarchy(o, name)
        _cache[name] = (o, H, mg_cases.vectors(o.Nc, float(np.abs(o.get("p_diag")).mean())))
    return _cache[name]


@pytest.mark.parametrize("name", list(mg_cases.CASES))
def test_oracle_hierarchy_has_the_reference_shapes_and_operator(oracle, name):
    o, H, v = setup(oracle, name)
    assert H.shapes == mg_ref.shapes(*mg_cases.CASES[name]["dims"])
    assert mg_cases.rel(o.apply_p(v["random"]), H.apply(v["random"])) <= 1e-14


def test_each_case_reaches_the_branch_it_was_chosen_for():
    sh = {n: mg_ref.shapes(*c["dims"]) for n, c in mg_cases.CASES.items()}
    assert len(sh["4x4x4"]) == 1 and len(sh["8x8x8"]) == 2
    assert sh["16x16x4"][-1] == (8, 8, 2)                                        # 128 cells, z stride 64
    assert sh["16x16x5"][0][0] * sh["16x16x5"][0][1] * sh["16x16x5"][0][2] == 1280
    assert sh["20x20x20"][1:] == [(10, 10, 10), (5, 5, 5)]
    assert len(sh["40x12x6"]) == 4 and sh["40x12x6"][2] == (10, 3, 2)            # 60 cells, but an edge of 10
    assert sh["4x4x512"][1] == (2, 2, 256) and len(sh["4x4x512"]) == 7           # 1024 cells and six levels from level 1 on
    assert sh["13x9x7"][1] == (7, 5, 4) and sh["33x17x9"][1:3] == [(17, 9, 5), (9, 5, 3)]      # odd edges on the levels below, too


@pytest.mark.parametrize("name", list(mg_cases.CASES))
@pytest.mark.parametrize("rhs", ["random", "smooth"])
def test_oracle_precondition_matches_reference(oracle, name, rhs):
    o, H, v = setup(oracle, name)
    z_ref = H.precondition(v[rhs])
    d = mg_cases.rel(o.precondition(v[rhs]), z_ref)
    print(f"{name} {rhs}: |z_oracle - z_ref| / max|z_ref| = {d:.2e}")
    assert d <= TOL


@pytest.mark.parametrize("name", list(mg_cases.CASES))
def test_oracle_cut_pcg_matches_reference(oracle, name):
    _, H, v = setup(oracle, name)
    xs, res = mg_ref.pcg(H.apply, H.precondition, v["b"], v["x0"], max(mg_cases.CUTS))
    for cut in mg_cases.CUTS:
        o = mg_cases.stepped(oracle.fv_case, oracle.FvSolver, name, p_max_iter=cut)
        x, it = o.solve_p(v["b"], v["x0"])
        st = o.stats()
        o.close()
        x_scale = float(np.abs(xs[cut - 1]).max())
        d = mg_cases.rel(x, xs[cut - 1])
        rs = mg_cases.residual_scale(H, x_scale, v["b"], v["x0"])
        print(f"{name} cut {cut}: dx = {d:.2e}, residuals {st['p_initial_residual']:.15e} {float(res[0]):.15e} | {st['p_final_residual']:.15e} {float(res[cut]):.15e}")
        # (one level: M^-1 = A^-1, the first iteration solves the system and a later one may meet a residual under p_tol = 1e-30)
        assert it == cut or (len(H.levels) == 1 and 1 <= it < cut and st["p_final_residual"] < 1e-30)
        assert d <= TOL
        assert abs(st["p_initial_residual"] - float(res[0])) <= TOL * rs
        assert abs(st["p_final_residual"] - float(res[cut])) <= TOL * rs


@pytest.mark.parametrize("name", list(mg_cases.CASES))
def test_reference_cycle_is_symmetric_positive_definite_and_contracts(oracle, name):
    _, H, v = setup(oracle, name)
    a, b = np.asarray(v["random"], np.longdouble), np.asarray(v["smooth"], np.longdouble)
    Ma, Mb = H.precondition(a), H.precondition(b)
    assert abs(Ma @ b - Mb @ a) <= 1e-15 * np.sqrt(Ma @ Ma) * np.sqrt(b @ b)
    assert Ma @ a > 0 and Mb @ b > 0
    # One cycle on an error with every frequency in it (the random vector).  This is a condition on the cycle as PCG meets it, not the norm of its error
    # operator: aggregation with piecewise-constant transfer and the half-weighted Galerkin product over-corrects the modes that are smooth inside an
    # aggregate, and repeating the cycle on its own output (the power method) climbs to 0.5 - 0.95 on these cases.
    rho = H.contraction(a)
    print(f"{name}: energy-norm contraction of one cycle = {rho:.3f}")
    assert rho <= 0.25


def test_single_level_cycle_is_the_exact_solve(oracle):
    o, H, v = setup(oracle, "4x4x4")
    assert len(H.levels) == 1
    for rhs in ("random", "smooth"):
        r = v[rhs]
        for z in (o.precondition(r), H.precondition(r)):
            assert np.abs(H.apply(z) - r).max() <= 1e-12 * np.abs(r).sum()


def test_reference_sees_a_missing_or_misplaced_reference_term(oracle):
    """what the parity tests rest on: dropping the reference cell's point term from the coarse operators, or giving it to the neighbouring aggregate, moves
    the cycle's result by tenths of its size -- eleven orders of magnitude over the bound"""
    o, H, v = setup(oracle, "13x9x7")
    ops = [o.get(nm) for nm in ("p_diag", "p_ux", "p_uy", "p_uz")]
    z = H.precondition(v["random"])
    without = mg_ref.Hierarchy(*ops, H.dims, None).precondition(v["random"])
    moved = mg_ref.Hierarchy(*ops, H.dims, 408, ref_aggregate=lambda l, at: (max(at[0] - 1, 0), at[1], at[2])).precondition(v["random"])
    assert mg_cases.rel(without, z) > 0.1 and mg_cases.rel(moved, z) > 0.05
    bent = [a.copy() for a in ops]
    bent[1][300] *= 1.0 + 1e-6
    assert mg_cases.rel(mg_ref.Hierarchy(*bent, H.dims, 408).precondition(v["random"]), z) > 1e-9
