"""Heat transfer in a case directory (no GPU): constant/couplingProperties `heatTransfer { ... }`, the start time's T | T.<phase>, div(phi,T) | div(alphaPhic,T) and
solvers.T land in fy_case_desc.thermal through the one read_coupling_properties path; no dictionary means all zero; what the solver cannot run is refused with
the file, the entry and the accepted words in the message.  Copies of tests/golden/cases."""
import os
import re
import shutil

import numpy as np
import pytest

from field_average_cases import case_copy

HEADER = "FoamFile { version 2.0; format ascii; class dictionary; location \"constant\"; object couplingProperties; }\n"
FULL = "heatTransfer { active on; nusseltModel %s; Cp 4180; kappa 0.6; Prt 0.9; particleTemperature 350; }\n"
PATCHES = {"bed_pimple": ("T.water", ["bottom", "top", "walls"]), "cavity_ico": ("T", ["movingWall", "fixedWalls"])}


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def write_T(dst, name, internal="uniform 300", entries=None):
    fname, patches = PATCHES[name]
    entries = entries or {}
    body = "".join(f"    {p} {{ {entries.get(p, 'type zeroGradient;')} }}\n" for p in patches)
    (dst / "0" / fname).write_text(f"FoamFile {{ version 2.0; format ascii; class volScalarField; object {fname}; }}\ndimensions [0 0 0 1 0 0 0];\n"
                                   f"internalField {internal};\nboundaryField\n{{\n{body}}}\n")


def edit(path, pattern, repl):
    text = path.read_text()
    new, n = re.subn(pattern, repl, text, count=1, flags=re.S)
    assert n == 1, (path, pattern)
    path.write_text(new)


def heat_case(tmp_path, name, coupling=FULL % "RanzMarshall", div="bounded Gauss upwind", solvers=True, T=True, kind="block", **tkw):
    """a copy of a golden case with heat transfer switched on in all four places"""
    dst = case_copy(tmp_path, name, kind)
    (dst / "constant/couplingProperties").write_text(HEADER + coupling)
    fname = PATCHES[name][0]
    if T:
        write_T(dst, name, **tkw)
    if div:
        term = "div(alphaPhic,T)" if name == "bed_pimple" else "div(phi,T)"
        edit(dst / "system/fvSchemes", r"(divSchemes\s*\{)", rf"\1\n    {term} {div};")
    if solvers:
        edit(dst / "system/fvSolution", r"(solvers\s*\{)", rf"\1\n    {fname} {{ solver smoothSolver; smoother symGaussSeidel; tolerance 1e-9; relTol 0.01; maxIter 77; }}")
    return dst


def thermal_of(prod, dst, solver):
    fc = prod.FoamCase(dst, solver)
    t = fc.case.thermal
    out = dict(on=t.on, cp=t.cp, kappa=t.kappa, prt=t.prt, law=t.nusselt_law, T_initial=t.T_initial, bc=list(t.T_bc), val=list(t.T_value), scheme=t.T_convection_scheme,
               tol=t.T_tol, rel=t.T_rel_tol, it=t.T_max_iter, Tp=t.particle_temperature)
    T0 = fc.initial_T() if t.on else None
    fc.close()
    return out, T0


def test_no_dictionary_means_all_zero(prod, tmp_path):
    for name, solver in (("bed_pimple", prod.FY_SOLVER_PIMPLE), ("cavity_ico", prod.FY_SOLVER_ICO)):
        dst = case_copy(tmp_path, name, "block")
        t, _ = thermal_of(prod, dst, solver)
        assert t == dict(on=0, cp=0, kappa=0, prt=0, law=0, T_initial=0, bc=[0] * 6, val=[0.0] * 6, scheme=0, tol=0, rel=0, it=0, Tp=0)
        (dst / "constant/couplingProperties").write_text(HEADER + "dragModel reference;\nheatTransfer { active off; Cp 4180; kappa 0.6; }\n")
        assert thermal_of(prod, dst, solver)[0]["on"] == 0
        fc = prod.FoamCase(dst, solver)
        with pytest.raises(prod.FoamYadeError):
            fc.initial_T()
        fc.close()


def test_each_word_lands_in_the_descriptor(prod, tmp_path):
    dst = heat_case(tmp_path, "bed_pimple", coupling="dragModel Beetstra;\n" + FULL % "Gunn",
                    entries={"bottom": "type fixedValue; value uniform 320;", "top": "type fixedValue; value uniform 290;"})
    t, T0 = thermal_of(prod, dst, prod.FY_SOLVER_PIMPLE)
    assert (t["on"], t["cp"], t["kappa"], t["prt"], t["law"], t["Tp"]) == (1, 4180.0, 0.6, 0.9, prod.NUSSELT_GUNN, 350.0)
    assert t["T_initial"] == 300.0 and (T0 == 300.0).all() and T0.size == 12 * 12 * 24
    # bottom is ZMIN, top ZMAX, the walls the four sides
    assert t["bc"] == [0, 0, 0, 0, 1, 1] and t["val"] == [0, 0, 0, 0, 320.0, 290.0]
    assert (t["scheme"], t["tol"], t["rel"], t["it"]) == (prod.FY_CONVECTION_UPWIND, 1e-9, 0.01, 77)
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.case.drag_law == prod.DRAG_BEETSTRA           # the rest of the file is still read
    fc.close()
    # defaults: RanzMarshall, Prt 1, particleTemperature 0, Gauss linear; a nonuniform internal field
    vals = 280.0 + 0.01 * np.arange(16.0 ** 3)
    ico = heat_case(tmp_path, "cavity_ico", coupling="heatTransfer { Cp 1000; kappa 0.03; }\n", div="Gauss linear",
                    internal="nonuniform List<scalar> 4096\n(\n" + "\n".join(repr(float(v)) for v in vals) + "\n)")
    t, T0 = thermal_of(prod, ico, prod.FY_SOLVER_ICO)
    assert (t["on"], t["cp"], t["kappa"], t["prt"], t["law"], t["Tp"], t["scheme"]) == (1, 1000.0, 0.03, 1.0, prod.NUSSELT_RANZ_MARSHALL, 0.0, prod.FY_CONVECTION_LINEAR)
    np.testing.assert_array_equal(T0, vals)
    # no div entry for T: a usable `default` gives its family ...
    dflt = heat_case(tmp_path / "b", "bed_pimple", div=None)
    edit(dflt / "system/fvSchemes", r"default\s+none;", "default Gauss upwind;")
    assert thermal_of(prod, dflt, prod.FY_SOLVER_PIMPLE)[0]["scheme"] == prod.FY_CONVECTION_UPWIND
    # ... and a named entry wins over `default` whichever comes first
    for first in (True, False):
        dst = heat_case(tmp_path / f"order{int(first)}", "bed_pimple", div=None)
        named, default = "div(alphaPhic,T) Gauss linear;", "default Gauss upwind;"
        edit(dst / "system/fvSchemes", r"default\s+none;", f"{named}\n    {default}" if first else f"{default}\n    {named}")
        assert thermal_of(prod, dst, prod.FY_SOLVER_PIMPLE)[0]["scheme"] == prod.FY_CONVECTION_LINEAR, first


def test_field_average_takes_the_temperature_file(prod, tmp_path):
    from field_average_cases import ON, add_functions, field_average
    dst = heat_case(tmp_path, "bed_pimple")
    add_functions(dst, field_average([("T.water", ON), ("p", ON)]))
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.case.average.as_list() == [("T", True, "time"), ("p", True, "time")]
    fc.close()
    cold = case_copy(tmp_path / "cold", "bed_pimple", "block")
    add_functions(cold, field_average([("T.water", ON)]))
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(cold, prod.FY_SOLVER_PIMPLE)          # no heat transfer: no T to average
    assert "error 5" in str(e.value) and "T.water" in str(e.value)


REFUSALS = [
    ("cavity_ico", dict(coupling=FULL % "Gunn"), "constant/couplingProperties", "nusseltModel", ["RanzMarshall"]),
    ("bed_pimple", dict(coupling=FULL % "Whitaker"), "constant/couplingProperties", "nusseltModel", ["RanzMarshall", "Gunn"]),
    ("bed_pimple", dict(coupling="heatTransfer { active on; kappa 0.6; }\n"), "constant/couplingProperties", "Cp", ["J/kg/K"]),
    ("bed_pimple", dict(coupling="heatTransfer { active on; Cp 4180; }\n"), "constant/couplingProperties", "kappa", ["W/m/K"]),
    ("bed_pimple", dict(coupling="heatTransfer { active perhaps; Cp 4180; kappa 0.6; }\n"), "constant/couplingProperties", "active", ["on", "off"]),
    ("bed_pimple", dict(coupling="heatTransfer { active on; Cp 4180; kappa 0.6; radiation on; }\n"), "constant/couplingProperties", "radiation", ["nusseltModel", "particleTemperature"]),
    ("bed_pimple", dict(T=False), "0/T.water", "heatTransfer", ["zeroGradient", "fixedValue"]),
    ("cavity_ico", dict(T=False), "0/T", "heatTransfer", ["zeroGradient", "fixedValue"]),
    ("bed_pimple", dict(entries={"top": "type inletOutlet; inletValue uniform 300; value uniform 300;"}), "0/T.water", "inletOutlet", ["zeroGradient", "fixedValue"]),
    ("bed_pimple", dict(entries={"top": "type fixedValue;"}), "0/T.water", "top", ["value uniform"]),
    ("bed_pimple", dict(div="Gauss vanLeer"), "system/fvSchemes", "div(alphaPhic,T)", ["linear", "upwind"]),
    ("bed_pimple", dict(div=None), "system/fvSchemes", "div(alphaPhic,T)", ["default none", "linear", "upwind"]),
    ("cavity_ico", dict(div=None), "system/fvSchemes", "div(phi,T)", ["default none", "linear", "upwind"]),
    ("bed_pimple", dict(solvers=False), "system/fvSolution", "T.water", ["tolerance", "maxIter"]),
    ("bed_pimple", dict(kind="general"), "constant/couplingProperties", "heatTransfer", ["general mesh", "off"]),
]


@pytest.mark.parametrize("name,kw,file,entry,accepted", REFUSALS, ids=[f"{q}-{r[0]}-{r[2].split('/')[-1]}-{r[3]}" for q, r in enumerate(REFUSALS)])
def test_what_cannot_run_is_refused_by_name(prod, tmp_path, name, kw, file, entry, accepted):
    dst = heat_case(tmp_path, name, **kw)
    solver = prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO
    with pytest.raises(prod.FoamYadeError) as e:
        (prod.GeneralFoamCase if kw.get("kind") == "general" else prod.FoamCase)(dst, solver)
    msg = str(e.value)
    assert "error 5" in msg, msg                             # FY_ERR_UNSUPPORTED
    assert file in msg and entry in msg, msg
    for w in accepted:
        assert w in msg, (w, msg)


def test_a_decomposed_case_refuses_heat_transfer(prod, tmp_path):
    dst = heat_case(tmp_path, "bed_pimple")
    for r in range(2):
        os.makedirs(dst / f"processor{r}" / "0")
        for f in ("U.water", "p", "T.water"):
            shutil.copy(dst / "0" / f, dst / f"processor{r}" / "0" / f)
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE, processor=(0, 2))
    assert "error 5" in str(e.value) and "constant/couplingProperties" in str(e.value) and "heatTransfer" in str(e.value) and "z-slabs" in str(e.value)
