"""controlDict `functions`: the fieldAverage object of a case directory, read by one function for block and general cases and carried as the `average`
descriptor appended to fy_case_desc / fy_ldu_case (all zero = no averaging); what fieldAverage offers beyond running means and prime2Means is refused by
name; function objects of other types are opened and not run.  Plus the numpy restatement's recurrence against its closed forms.  Copies of tests/golden/cases."""
import shutil

import numpy as np
import pytest

import field_average_ref as far
from field_average_cases import KINDS, MEAN, ON, add_functions, case_copy, field_average, open_case


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def average_of(prod, dst, solver, kind):
    """(items, start_after, stop_after, ignored function objects) as the descriptor a solver would be made from carries them"""
    fc = open_case(prod, dst, solver, kind)
    av = fc.ldu_case.average if kind == "general" else fc.case.average
    out = (av.as_list(), av.start_after, av.stop_after, list(fc.ignored_functions))
    fc.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_the_descriptor_carries_items_bases_and_window(prod, tmp_path, kind):
    dst = case_copy(tmp_path, "bed_pimple", kind)
    add_functions(dst, field_average([("U.water", ON), ("p", "mean on; prime2Mean on; base iteration;"), ("alpha.water", MEAN), ("uParticle", MEAN),
                                      ("uSource", "mean off; prime2Mean off; base time;")],
                                     "timeStart 0.0005; timeEnd 0.0015; writeControl writeTime; executeControl timeStep; executeInterval 1; restartOnRestart off; restartOnOutput off; periodicRestart no;"))
    items, start_after, stop_after, ignored = average_of(prod, dst, prod.FY_SOLVER_PIMPLE, kind)
    assert items == [("U", True, "time"), ("p", True, "iteration"), ("alpha", False, "time"), ("uParticle", False, "time")]       # (both moments off: dropped)
    assert start_after == 0.0005 and stop_after == 0.0015 and ignored == []
    ico = case_copy(tmp_path, "cavity_ico", kind)
    add_functions(ico, field_average([("U", MEAN), ("p", ON), ("uSource", MEAN)], "timeStart 0;"))
    assert average_of(prod, ico, prod.FY_SOLVER_ICO, kind) == ([("U", False, "time"), ("p", True, "time"), ("uSource", False, "time")], 0.0, 0.0, [])


@pytest.mark.parametrize("kind", KINDS)
def test_no_functions_means_no_averaging(prod, tmp_path, kind):
    assert average_of(prod, case_copy(tmp_path, "bed_pimple", kind), prod.FY_SOLVER_PIMPLE, kind) == ([], 0.0, 0.0, [])
    assert average_of(prod, case_copy(tmp_path, "cavity_ico", kind), prod.FY_SOLVER_ICO, kind) == ([], 0.0, 0.0, [])
    assert prod.CaseDesc().average.n_items == 0 and prod.LduCase().average.n_items == 0          # a zero-initialised descriptor averages nothing
    assert prod.case_defaults(prod.FY_SOLVER_PIMPLE).average.n_items == 0


@pytest.mark.parametrize("kind", KINDS)
def test_disabled_objects_and_other_types_are_opened_and_not_run(prod, tmp_path, kind):
    dst = case_copy(tmp_path, "bed_pimple", kind)
    add_functions(dst, field_average([("U.water", ON)], "enabled false;", name="off1") +
                  "    probes1 { type probes; libs (\"libsampling.so\"); fields (p); probeLocations ((0 0 0.01)); }\n" +
                  field_average([("p", MEAN)], name="avg2") +
                  "    co { type CourantNo; }\n")
    items, _, _, ignored = average_of(prod, dst, prod.FY_SOLVER_PIMPLE, kind)
    assert items == [("p", False, "time")]
    assert ignored == ["probes1 (type probes)", "co (type CourantNo)"]


REFUSALS = [
    # (case, the functions dictionary's body, what the message must name, accepted words it must list)
    ("bed_pimple", field_average([("U.water", ON)], "window 0.001;"), ["window"], ["no window"]),
    ("bed_pimple", field_average([("U.water", ON + " window 10;")]), ["window", "U.water"], ["no window"]),
    ("bed_pimple", field_average([("U.water", ON)], "restartOnOutput on;"), ["restartOnOutput"], ["off"]),
    ("bed_pimple", field_average([("U.water", ON)], "periodicRestart on; restartPeriod 0.002;"), ["periodicRestart"], ["off"]),
    ("bed_pimple", field_average([("T", ON)]), ["unknown field", "'T'"], ["U.water", "p", "alpha.water", "uParticle", "uSource"]),
    ("bed_pimple", field_average([("k.water", ON)]), ["no field", "k.water"], ["U.water", "p", "alpha.water"]),
    ("bed_pimple", field_average([("U", ON)]), ["no field", "'U'"], ["U.water"]),
    ("cavity_ico", field_average([("alpha.water", ON)]), ["no field", "alpha.water"], ["U", "p", "uSource"]),
    ("cavity_ico", field_average([("uParticle", ON)]), ["no field", "uParticle"], ["U", "p", "uSource"]),
    ("bed_pimple", field_average([("p", "mean on; prime2Mean on; base ensemble;")]), ["base", "ensemble"], ["time", "iteration"]),
    ("bed_pimple", field_average([("p", "mean off; prime2Mean on; base time;")]), ["prime2Mean", "mean"], ["mean on"]),
    ("bed_pimple", field_average([("p", ON)], "writeControl timeStep; writeInterval 3;"), ["writeControl", "timeStep"], ["writeTime", "outputTime"]),
    ("bed_pimple", field_average([("p", ON)], "executeControl runTime;"), ["executeControl", "runTime"], ["timeStep"]),
    ("bed_pimple", field_average([("p", ON)], "executeControl timeStep; executeInterval 2;"), ["executeInterval"], ["1"]),
    ("bed_pimple", field_average([("p", ON)], name="a1") + field_average([("U.water", ON)], name="a2"), ["second", "fieldAverage", "a1"], ["one"]),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,body,named,accepted", REFUSALS)
def test_what_is_not_implemented_is_refused_by_name(prod, tmp_path, kind, name, body, named, accepted):
    dst = case_copy(tmp_path, name, kind)
    add_functions(dst, body)
    with pytest.raises(prod.FoamYadeError) as e:
        average_of(prod, dst, prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO, kind)
    msg = str(e.value)
    assert "error 5" in msg                                      # FY_ERR_UNSUPPORTED
    assert "system/controlDict" in msg and "functions." in msg and "accepted" in msg
    for w in named + accepted:
        assert w in msg, (w, msg)


def test_a_field_listed_twice_is_refused(prod, tmp_path):
    """(a case has eight averageable fields at the most, FY_AVERAGE_MAX_ITEMS: a ninth entry is necessarily a repeated one)"""
    dst = case_copy(tmp_path, "bed_pimple", "block")
    add_functions(dst, field_average([("U.water", ON), ("p", ON), ("p", ON)]))
    with pytest.raises(prod.FoamYadeError) as e:
        average_of(prod, dst, prod.FY_SOLVER_PIMPLE, "block")
    assert "twice" in str(e.value) and "functions.fieldAverage1.fields.p" in str(e.value)


def test_fieldaverage_in_a_decomposed_case_is_refused(prod, tmp_path):
    """foamYadeHip_mpi -parallel on processor directories opens each with fy_foam_case_open_processor: fieldAverage is refused there by name"""
    dst = case_copy(tmp_path, "bed_pimple", "block")
    add_functions(dst, field_average([("p", ON)]))
    for r in range(2):
        (dst / f"processor{r}").mkdir()
        shutil.copytree(dst / "0", dst / f"processor{r}" / "0")
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE, processor=(0, 2))
    msg = str(e.value)
    assert "error 5" in msg and "fieldAverage" in msg and "-parallel" in msg and "accepted" in msg


@pytest.mark.parametrize("base", ["time", "iteration"])
def test_recurrence_equals_the_closed_forms(base):
    """8 samples with unequal deltaT: the running update is the weighted mean and the weighted mean of squares minus the mean squared.  The two differ by
    rounding only, about n eps = 2e-15 of the data's scale; the bar leaves three decades"""
    rng = np.random.default_rng(7)
    n, steps = 500, 8
    dts = rng.uniform(0.5e-3, 2e-3, steps)
    xs = [rng.normal(0.3, 1.0, n) for _ in range(steps)]
    vs = [rng.normal(0.0, 2.0, (n, 3)) + np.array([1.0, -2.0, 0.5]) for _ in range(steps)]
    s, v = far.Item((n,), True, base), far.Item((n, 3), True, base)
    for x, u, dt in zip(xs, vs, dts):
        s.add(x, dt); v.add(u, dt)
    assert s.N == steps and v.N == steps and abs(s.T - dts.sum()) < 1e-15
    for item, data in ((s, xs), (v, vs)):
        m, P = far.closed_form(data, dts, base)
        scale = max(np.abs(d).max() for d in data)
        assert np.abs(item.m - m).max() <= 1e-12 * scale
        assert np.abs(item.P - P).max() <= 1e-12 * scale ** 2
    # the first sample needs no special case: a = 0, b = 1 gives m = x and P = 0 exactly
    one = far.Item((n, 3), True, base)
    one.add(vs[0], dts[0])
    assert np.array_equal(one.m, vs[0]) and not one.P.any()
    # a mean-only item's mean is the same recurrence
    mo = far.Item((n,), False, base)
    for x, dt in zip(xs, dts):
        mo.add(x, dt)
    assert np.array_equal(mo.m, s.m) and mo.P is None
