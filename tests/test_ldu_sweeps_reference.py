"""The CPU side of tests/ldu_sweep_cases.py, without a GPU: oracle/ldu_oracle.cpp is one source in two widths, and this file holds the two to each other.

  * the double build (liboracle.so) is the oracle it was before it learned to compile in long double: U, p and phi of every laminar case reproduce the SHA-256
    recorded from the build of the commit before (tests/golden/ldu_oracle_bits.json: ldu_sweep_cases.oracle_bits over LAMINAR_SINGLE, one thread; the turbulent
    cases go through pow / cbrt / sqrt of whatever libm is present and are left out);
  * the wide build (liboracle_ld.so) really computes with a 64-bit mantissa, and says so loudly where it does not;
  * with every count frozen both builds do the same number of iterations, and the double build stays within 1e-17 .. 1e-12 of the wide one in every field
    group over the whole case list (seeded random coupling fields) -- the window tests/test_ldu_sweeps_parity.py relies on for its device bound of
    50 x max(e_oracle, 2^-52);
  * that bound sees a coefficient wrong in the ninth digit: the double build with nu scaled by 1 + 1e-9 lands above it;
  * and the other convection scheme of k on a through-flow lands a factor 1e8 above it (the two solvers' defaults differ: a case names its scheme).
Measured: DESIGN.md, parity section."""
import json
import os

import numpy as np
import pytest

import ldu_sweep_cases as lc

NAMES = list(lc.CASES)
_runs, _env = {}, []


def coupling_of(c):
    return [lc.random_coupling(c, s) for s in range(2)]


def both_builds(oracle, name):
    """(double build, wide build): per step (fields, stats), once per case"""
    if name not in _runs:
        c = lc.CASES[name]
        cpl = coupling_of(c)
        _runs[name] = (lc.run_oracle(oracle, c, cpl, wide=False), lc.run_oracle(oracle, c, cpl, wide=True))
    return _runs[name]


def envelope(oracle):
    """e_oracle over the whole list, printed case by case; measured once"""
    if not _env:
        e = lc.Envelope()
        for name in NAMES:
            dbl, wide = both_builds(oracle, name)
            for step in range(2):
                w = e.add(name, step, lc.distances(lc.CASES[name], dbl[step], wide[step]))
                print(f"{name:34s} step {step + 1}  " + "  ".join(f"{g} {w[g][0]:.2e} {w[g][1]}" for g in lc.GROUPS))
        print(e.report())
        _env.append(e)
    return _env[0]


def test_wide_build_has_a_64_bit_mantissa_and_refuses_what_needs_double_storage(oracle):
    assert oracle._ldu_lib(wide=True).orc_ldu_real_mant_dig() == 64 and oracle._ldu_lib().orc_ldu_real_mant_dig() == 53
    c = lc.CASES["pimple_wavy"]
    o = lc.oracle_solver(oracle, c, wide=True)
    with pytest.raises(RuntimeError, match="long-double build"):
        o.view("U")
    x = np.random.RandomState(1).rand(3 * o.nc)
    o.set("uSource", x)
    np.testing.assert_array_equal(o.get("uSource"), x)          # doubles cross the interface unchanged
    o.close()
    o = lc.oracle_solver(oracle, c, wide=False)
    o.set("uSource", x)
    np.testing.assert_array_equal(o.view("uSource"), x)         # (the double build: get / set and the view are one storage)
    o.close()


@pytest.mark.parametrize("name", lc.LAMINAR_SINGLE)
def test_double_build_reproduces_the_recorded_bits(oracle, name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ldu_oracle_bits.json")) as f:
        want = json.load(f)
    assert set(want) == set(lc.LAMINAR_SINGLE)
    assert lc.oracle_bits(oracle, name) == want[name]


@pytest.mark.parametrize("name", NAMES)
def test_counts_are_frozen_and_every_compared_field_is_live(oracle, name):
    c = lc.CASES[name]
    for side in both_builds(oracle, name):
        for fields, st in side:
            assert lc.counts_ok(c, st), (lc.expected_counts(c), st)
            for nm, v in fields.items():
                assert np.isfinite(v).all() and (np.abs(v).max() > 0) == (nm not in c["zero"]), nm
    cpl = coupling_of(c)[0]
    if c["solver"] == 1:
        assert cpl["alpha"].min() < 0.9 and cpl["uSourceDrag"].min() < 0
    assert set(lc.NEVER_OMITTED) <= set(lc.compared(c))


def test_every_omission_carries_its_reason():
    for c in lc.CASES.values():
        for nm, why in lc.omitted(c).items():
            assert nm in lc.GROUP_OF and len(why) > 10, (c["name"], nm)
        assert set(c["zero"]) <= set(lc.compared(c)), c["name"]


def test_the_list_reaches_the_blocks_it_names():
    """the wavy mesh: more than one 256-thread block with a ragged last one on cells, faces and boundary faces; the chain: two internal faces"""
    n, nf, ni = lc.counts_of(lc.mesh_of(lc.CASES["ico_wavy"]))
    for count in (n, ni, nf - ni, nf):
        assert count > 256 and count % 256
    assert lc.counts_of(lc.mesh_of(lc.CASES["ico_chain"])) == (3, 16, 2)
    assert lc.counts_of(lc.mesh_of(lc.CASES["ico_refined"]))[0] == 960 and max(lc.counts_of(lc.mesh_of(c))[0] for c in lc.CASES.values()) <= 1000


def test_double_build_stays_within_rounding_of_the_wide_one(oracle):
    """e_oracle per group and step: the largest distance of the double build from the wide one over the whole case list"""
    envelope(oracle).check_window()


@pytest.mark.parametrize("name", lc.SENSITIVITY)
def test_a_coefficient_wrong_in_the_ninth_digit_lands_above_the_bound(oracle, name):
    """the double build with nu scaled by 1 + 1e-9 against the wide build with nu as it is: what is assembled from nu leaves the bound the device gets"""
    e = envelope(oracle)
    c = lc.CASES[name]
    off = lc.run_oracle(oracle, c, coupling_of(c), wide=False, nu_factor=1.0 + 1e-9)
    _, wide = both_builds(oracle, name)
    for step in range(2):
        v, nm = lc.worst(lc.distances(c, off[step], wide[step]))["assembled"]
        print(f"{name} step {step + 1}: assembled {v:.2e} ({nm})  bound {e.bound('assembled', step):.2e}")
        assert v > e.bound("assembled", step), (step, nm, v)


def test_the_other_k_scheme_lands_far_above_the_bound(oracle):
    """the double build with upwind convection of k against the wide build with the case's linear one, on the through-flow with a k inlet: k leaves the bound the
    device gets in its group by more than a factor 1000 (expected: 1e-3 or more against a bound near 1e-11) -- a solver that ran its own default instead of the
    named scheme cannot pass the parity test"""
    e = envelope(oracle)
    name = "pimple_through_flow_kEqn_linear_k_inlet"
    c = lc.CASES[name]
    assert c["kw"]["k_convection_scheme"] == 0
    other = dict(c, kw=dict(c["kw"], k_convection_scheme=1))
    off = lc.run_oracle(oracle, other, coupling_of(c), wide=False)
    _, wide = both_builds(oracle, name)
    for step in range(2):
        v = lc.distances(c, off[step], wide[step])[lc.GROUP_OF["k"]]["k"]
        bound = e.bound(lc.GROUP_OF["k"], step)
        print(f"{name} step {step + 1}: k {v:.2e}  bound {bound:.2e}")
        assert v > 1000.0 * bound, (step, v, bound)
