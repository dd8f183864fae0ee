"""The thermal loop in a case directory (no GPU): constant/couplingProperties `heatTransfer { ... particleCp; beta; TRef; }` lands in fy_case_desc.thermal, absent entries
leave zeros, and what cannot run is refused with the file and the entry in the message.  Copies of tests/golden/cases, through tests/test_heat_transfer_case.py's helpers."""
import pytest

from test_heat_transfer_case import heat_case

BASE = "heatTransfer { active on; Cp 4180; kappa 0.6; particleTemperature 350; %s }\n"


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def loop_of(prod, dst, solver):
    fc = prod.FoamCase(dst, solver)
    t = fc.case.thermal
    out = (t.on, t.particle_cp, t.beta, t.T_ref, t.particle_temperature)
    fc.close()
    return out


@pytest.mark.parametrize("name", ["cavity_ico", "bed_pimple"])
def test_the_three_entries_arrive(prod, tmp_path, name):
    solver = prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO
    dst = heat_case(tmp_path / "full", name, coupling=BASE % "particleCp 840; beta 2.07e-4; TRef 293.15;")
    assert loop_of(prod, dst, solver) == (1, 840.0, 2.07e-4, 293.15, 350.0)
    # absent entries leave zeros; each one stands alone (TRef without beta is harmless, beta 0 needs no TRef)
    assert loop_of(prod, heat_case(tmp_path / "none", name, coupling=BASE % ""), solver) == (1, 0.0, 0.0, 0.0, 350.0)
    assert loop_of(prod, heat_case(tmp_path / "cp", name, coupling=BASE % "particleCp 840;"), solver) == (1, 840.0, 0.0, 0.0, 350.0)
    assert loop_of(prod, heat_case(tmp_path / "tref", name, coupling=BASE % "TRef 300;"), solver) == (1, 0.0, 0.0, 300.0, 350.0)
    assert loop_of(prod, heat_case(tmp_path / "b0", name, coupling=BASE % "beta 0;"), solver) == (1, 0.0, 0.0, 0.0, 350.0)
    assert loop_of(prod, heat_case(tmp_path / "neg", name, coupling=BASE % "beta -1e-4; TRef 0;"), solver) == (1, 0.0, -1e-4, 0.0, 350.0)


REFUSALS = [
    ("particleCp copper;", "particleCp", ["J/kg/K"]),
    ("particleCp -840;", "particleCp", ["not negative"]),
    ("beta large; TRef 300;", "beta", ["1/K"]),
    ("beta 2e-4;", "beta", ["TRef"]),
    ("radiation on;", "radiation", ["particleTemperature, particleCp, beta, TRef"]),
    ("particleCP 840;", "particleCP", ["particleTemperature, particleCp, beta, TRef"]),
]


@pytest.mark.parametrize("name", ["cavity_ico", "bed_pimple"])
@pytest.mark.parametrize("entries,entry,words", REFUSALS, ids=[f"{q}-{r[1]}" for q, r in enumerate(REFUSALS)])
def test_what_cannot_run_is_refused_by_name(prod, tmp_path, name, entries, entry, words):
    dst = heat_case(tmp_path, name, coupling=BASE % entries)
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO)
    msg = str(e.value)
    assert "error 5" in msg, msg                             # FY_ERR_UNSUPPORTED
    assert "constant/couplingProperties" in msg and f"heatTransfer.{entry}" in msg, msg
    for w in words:
        assert w in msg, (w, msg)
