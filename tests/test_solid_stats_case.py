"""The solid-phase statistics in a case directory: constant/couplingProperties `solidStatistics on | off;` lands in fy_case_desc.solid_stats / fy_ldu_case.solid_stats
through the one read_coupling_properties path (CPU), fieldAverage and volFieldValue then take the new fields' names, and foamYadeHip writes them with every time
directory (GPU).  Copies of tests/golden/cases."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_coupling_properties import HEADER, KINDS, case_copy, write
from field_average_cases import field_average
from test_heat_transfer_case import heat_case
from test_monitors_case import vol

FILES = {"nParticle": ("volScalarField", "[0 -3 0 0 0 0 0]"), "solidFraction": ("volScalarField", "[0 0 0 0 0 0 0]"), "uSolid": ("volVectorField", "[0 1 -1 0 0 0 0]"),
         "granularTemperature": ("volScalarField", "[0 2 -2 0 0 0 0]"), "dSauter": ("volScalarField", "[0 1 0 0 0 0 0]")}
T_FILE = {"TParticle": ("volScalarField", "[0 0 0 1 0 0 0]")}


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def read(prod, dst, solver, kind):
    fc = prod.GeneralFoamCase(dst, solver) if kind == "general" else prod.FoamCase(dst, solver)
    out = fc.ldu_case.solid_stats if kind == "general" else fc.case.solid_stats
    fc.close()
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["bed_pimple", "cavity_ico"])
def test_the_entry_lands_in_the_descriptor(prod, tmp_path, kind, name):
    solver = prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO
    dst = case_copy(tmp_path, name, kind)
    assert read(prod, dst, solver, kind) == 0                                    # no file
    for word, value in (("on", 1), ("off", 0), ("true", 1), ("no", 0)):
        write(dst, f"solidStatistics {word};\n")
        assert read(prod, dst, solver, kind) == value, word
    write(dst, "dragModel reference;\n")
    assert read(prod, dst, solver, kind) == 0                                    # no entry
    assert prod.CaseDesc().solid_stats == 0 and prod.LduCase().solid_stats == 0 and prod.case_defaults(solver).solid_stats == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["bed_pimple", "cavity_ico"])
def test_a_word_that_is_no_boolean_is_refused_by_name(prod, tmp_path, kind, name):
    dst = case_copy(tmp_path, name, kind)
    write(dst, "solidStatistics perhaps;\n")
    with pytest.raises(prod.FoamYadeError) as e:
        read(prod, dst, prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO, kind)
    msg = str(e.value)
    assert "error 5" in msg and "constant/couplingProperties" in msg and "solidStatistics" in msg and "perhaps" in msg and "on | off" in msg, msg


def test_a_decomposed_case_refuses_it(prod, tmp_path):
    dst = case_copy(tmp_path, "bed_pimple", "block")
    write(dst, "solidStatistics on;\n")
    for r in range(2):
        os.makedirs(dst / f"processor{r}" / "0")
        for f in ("U.water", "p"):
            shutil.copy(dst / "0" / f, dst / f"processor{r}" / "0" / f)
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE, processor=(0, 2))
    assert "error 5" in str(e.value) and "constant/couplingProperties" in str(e.value) and "solidStatistics" in str(e.value) and "z-slabs" in str(e.value)
    write(dst, "solidStatistics off;\n")
    prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE, processor=(0, 2)).close()


FUNCTIONS = ("\nfunctions\n{\n" + vol("solids", ["solidFraction", "granularTemperature"], "volIntegrate") +
             field_average([("uSolid", "mean on; prime2Mean on; base time;"), ("dSauter", "mean on; prime2Mean off; base time;")]) + "}\n")


def test_function_objects_take_the_fields_only_while_it_is_on(prod, tmp_path):
    dst = case_copy(tmp_path, "bed_pimple", "block")
    ctl = dst / "system/controlDict"
    ctl.write_text(ctl.read_text() + FUNCTIONS)
    write(dst, "solidStatistics on;\n")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    av, mon = fc.case.average, fc.case.monitors
    assert [av.items[q].field.decode() for q in range(av.n_items)] == ["uSolid", "dSauter"] and av.items[0].prime2_mean == 1
    assert mon.n_objects == 1 and [mon.objects[0].fields[q].value.decode() for q in range(mon.objects[0].n_fields)] == ["solidFraction", "granularTemperature"]
    fc.close()
    for text, missing in (("solidStatistics off;\n", "solidFraction"), ("solidStatistics on;\n", "TParticle")):
        write(dst, text)
        if missing == "TParticle":
            ctl.write_text(ctl.read_text().replace("fields (solidFraction granularTemperature)", "fields (solidFraction TParticle)"))
        with pytest.raises(prod.FoamYadeError) as e:
            prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
        msg = str(e.value)
        assert "error 5" in msg and missing in msg and "accepted" in msg and "uParticle, uSource" in msg, msg
        assert ("granularTemperature" in msg.split("accepted")[1]) == (missing == "TParticle"), msg


def field_file(path):
    text = path.read_text()
    cls = re.search(r"class\s+(\w+);", text).group(1)
    dims = re.search(r"dimensions\s+(\[[^\]]*\]);", text).group(1)
    body = text[text.index("internalField"):text.index("boundaryField")]
    if "nonuniform" in body:
        nums = np.array([float(x) for x in re.findall(r"[-+0-9.eE]+", body[body.index("("):])])
    else:
        nums = np.array([float(x) for x in re.findall(r"[-+0-9.eE]+", body.split("uniform", 1)[1])])
    return cls, dims, nums, text[text.index("boundaryField"):]


@pytest.mark.gpu
@pytest.mark.parametrize("heat", [False, True], ids=["plain", "heatTransfer"])
def test_the_executable_writes_the_fields_with_every_time_directory(prod, tmp_path, heat):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yade-openfoam-coupling_amd", "bin", "foamYadeHip")
    if not os.path.exists(exe):
        pytest.fail("foamYadeHip has not been built: run __graft_entry__.build()")
    if heat:
        dst = heat_case(tmp_path, "bed_pimple", coupling="solidStatistics on;\nheatTransfer { active on; nusseltModel Gunn; Cp 1000; kappa 50; particleTemperature 350; }\n")
    else:
        dst = case_copy(tmp_path, "bed_pimple", "block")
        write(dst, "solidStatistics on;\n")
    want = dict(FILES, **(T_FILE if heat else {}))
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)      # fluid alone: no particles arrive
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("Coupling:")]
    assert len(lines) == 1 and "solidStatistics on" in lines[0], out.stdout
    times = sorted(d for d in os.listdir(dst) if re.fullmatch(r"[0-9.]+", d) and d != "0")
    assert len(times) >= 2, times
    for t in times:
        for name, (cls, dims) in want.items():
            assert os.path.exists(dst / t / name), (t, name)
            got_cls, got_dims, nums, boundary = field_file(dst / t / name)
            assert (got_cls, got_dims) == (cls, dims), (t, name, got_cls, got_dims)
            assert nums.size > 0 and (nums[1:] == 0.0).all(), (t, name)       # (the first number of a nonuniform list is its length)
            assert boundary.count("calculated") == 3 and ("uniform (0 0 0)" if name == "uSolid" else "uniform 0") in boundary, (t, name, boundary)
        if not heat:
            assert not os.path.exists(dst / t / "TParticle")
    # the same case without the entry writes none of them
    for t in times:
        shutil.rmtree(dst / t)
    (dst / "constant/couplingProperties").write_text(HEADER + ("heatTransfer { active on; nusseltModel Gunn; Cp 1000; kappa 50; particleTemperature 350; }\n" if heat else "// nothing\n"))
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("Coupling:")]
    for t in times:
        assert os.path.exists(dst / t / "p")
        for name in list(FILES) + list(T_FILE):
            assert not os.path.exists(dst / t / name), (t, name)
