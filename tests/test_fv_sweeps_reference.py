"""The CPU side of tests/fv_sweep_cases.py, without a GPU: oracle/fv_oracle.cpp is one source in two widths, and this file holds the two to each other.

  * the double build (liboracle.so) is the oracle it was before it learned to compile in long double: U, p and phi of every laminar case reproduce the SHA-256
    recorded from the build of the commit before (tests/golden/fv_oracle_bits.json: fv_sweep_cases.oracle_bits over LAMINAR_SINGLE, one thread; the turbulent
    cases go through pow / cbrt / log of whatever libm is present and are left out);
  * the wide build (liboracle_ld.so) really computes with a 64-bit mantissa, and says so loudly where it does not;
  * with every count frozen both builds do the same number of iterations, and the double build stays within 1e-17 .. 1e-12 of the wide one in every field
    group over the whole case list (seeded random coupling fields) -- the window tests/test_fv_sweeps_parity.py relies on for its device bound of
    50 x max(e_oracle, 2^-52);
  * the other convection scheme of k on a side that carries a flux lands a factor 1e8 above that bound (the two solvers' defaults differ: a case names its scheme).
Measured: DESIGN.md, parity section."""
import json
import os

import numpy as np
import pytest

import fv_sweep_cases as fc

NAMES = list(fc.CASES)
_runs, _env = {}, []


def coupling_of(c):
    return [fc.random_coupling(c, s) if c["couple"] else fc.no_coupling(c) for s in range(2)]


def both_builds(oracle, name):
    """(double build, wide build): per step (fields, stats), once per case"""
    if name not in _runs:
        c = fc.CASES[name]
        cpl = coupling_of(c)
        _runs[name] = (fc.run_oracle(oracle, c, cpl, wide=False), fc.run_oracle(oracle, c, cpl, wide=True))
    return _runs[name]


def test_wide_build_has_a_64_bit_mantissa_and_refuses_what_needs_double_storage(oracle):
    assert oracle._fv_lib(wide=True).orc_fv_real_mant_dig() == 64 and oracle._fv_lib().orc_fv_real_mant_dig() == 53
    c = fc.CASES["pimple_box_linear"]
    o = oracle.FvSolver(fc.oracle_case(oracle, c), wide=True)
    with pytest.raises(RuntimeError, match="long-double build"):
        o.view("U")
    with pytest.raises(RuntimeError, match="step_fields"):
        o.step(fc.records(c, 0))
    x = np.random.RandomState(1).rand(3 * o.Nc)
    o.set("uSource", x)
    np.testing.assert_array_equal(o.get("uSource"), x)          # doubles cross the interface unchanged
    o.close()


@pytest.mark.parametrize("name", fc.LAMINAR_SINGLE)
def test_double_build_reproduces_the_recorded_bits(oracle, name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fv_oracle_bits.json")) as f:
        want = json.load(f)
    assert set(want) == set(fc.LAMINAR_SINGLE)
    assert fc.oracle_bits(oracle, name) == want[name]


@pytest.mark.parametrize("name", NAMES)
def test_counts_are_frozen_and_every_compared_field_is_live(oracle, name):
    c = fc.CASES[name]
    for side in both_builds(oracle, name):
        for fields, st in side:
            assert fc.counts_ok(c, st), (fc.expected_counts(c), st)
            for nm, v in fields.items():
                assert np.isfinite(v).all() and (np.abs(v).max() > 0) == (nm not in c["zero"]), nm
    cpl = coupling_of(c)[0]
    if c["couple"]:
        assert np.abs(cpl["uSource"]).max() > 0 if c["solver"] == 0 else (cpl["alpha"].min() < 0.9 and cpl["uSourceDrag"].min() < 0)
    assert set(fc.NEVER_OMITTED) <= set(fc.compared(c)) or c["kw"].get("n_corr") == 0


def test_every_omission_carries_its_reason():
    for c in fc.CASES.values():
        for nm, why in fc.omitted(c).items():
            assert nm in fc.GROUP_OF and len(why) > 10, (c["name"], nm)


def envelope(oracle):
    """e_oracle over the whole list, printed case by case; measured once"""
    if not _env:
        e = fc.Envelope()
        for name in NAMES:
            dbl, wide = both_builds(oracle, name)
            for step in range(2):
                w = e.add(name, step, fc.distances(fc.CASES[name], dbl[step], wide[step]))
                print(f"{name:45s} step {step + 1}  " + "  ".join(f"{g} {w[g][0]:.2e} {w[g][1]}" for g in fc.GROUPS))
        print(e.report())
        _env.append(e)
    return _env[0]


def test_double_build_stays_within_rounding_of_the_wide_one(oracle):
    """e_oracle per group and step: the largest distance of the double build from the wide one over the whole case list"""
    envelope(oracle).check_window()


def test_the_other_k_scheme_lands_far_above_the_bound(oracle):
    """the double build with upwind convection of k against the wide build with the case's linear one, on the through-flow with a k inlet: k leaves the bound the
    device gets in its group by more than a factor 1000 (expected: 1e-3 or more against a bound near 1e-11) -- a solver that ran its own default instead of the
    named scheme cannot pass the parity test"""
    e = envelope(oracle)
    name = "pimple_c5_kEqn_linear_k_inlet"
    c = fc.CASES[name]
    assert c["kw"]["k_convection_scheme"] == 0
    other = dict(c, kw=dict(c["kw"], k_convection_scheme=1))
    off = fc.run_oracle(oracle, other, coupling_of(c), wide=False)
    _, wide = both_builds(oracle, name)
    for step in range(2):
        v = fc.distances(c, off[step], wide[step])[fc.GROUP_OF["k"]]["k"]
        bound = e.bound(fc.GROUP_OF["k"], step)
        print(f"{name} step {step + 1}: k {v:.2e}  bound {bound:.2e}")
        assert v > 1000.0 * bound, (step, v, bound)
