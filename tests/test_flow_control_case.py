"""constant/couplingProperties meanVelocityForce { ... }: flow-rate control of a case directory, carried in fy_ldu_case.flow_control; the restart file
<time>/uniform/meanVelocityForceProperties; foamYadeHip's line.  Copies of tests/golden/cases, made general (and periodic in x) the way test_coupling_properties.py and
test_ldu_case.py make theirs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import poly_meshes as pm

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "cases")
HEADER = "FoamFile { version 2.0; format ascii; class dictionary; location \"constant\"; object couplingProperties; }\n"


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def general_copy(tmp_path, name, periodic=True):
    """the golden case as a polyhedral mesh; periodic: its two x sides are a cyclic pair (left, right)"""
    dst = tmp_path / name
    shutil.copytree(os.path.join(CASES, name), dst)
    os.remove(dst / "system/blockMeshDict")
    if name == "cavity_ico":
        base = [("movingWall", [3]), ("fixedWalls", [2, 4, 5] if periodic else [0, 1, 2, 4, 5])]
        mesh = pm.hex_block(4, 4, 4, (0.1, 0.1, 0.1), patches=base + ([("left", [0]), ("right", [1])] if periodic else []))
        types = {}
    else:
        base = [("bottom", [4]), ("top", [5]), ("walls", [2, 3] if periodic else [0, 1, 2, 3])]
        mesh = pm.hex_block(4, 4, 8, (0.06, 0.06, 0.12), lambda P: P + np.array([-0.03, -0.03, 0.0]), patches=base + ([("left", [0]), ("right", [1])] if periodic else []))
        types = {"bottom": "patch", "top": "patch", "walls": "wall"}
    if periodic:
        mesh = pm.make_cyclic(mesh, [(len(base), len(base) + 1)])
    pm.write_poly_mesh_files(dst, mesh, types)
    if periodic:
        b = dst / "constant/polyMesh/boundary"
        t = b.read_text()
        i, j = t.index("left"), t.index("right")
        cyc = lambda txt, nbr: txt.replace("type            wall", "type            cyclic; neighbourPatch %s; transform translational" % nbr, 1)
        b.write_text(t[:i] + cyc(t[i:j], "right") + cyc(t[j:], "left"))
        assert b.read_text().count("cyclic") == 2
        for f in sorted((dst / "0").iterdir()):
            ft = f.read_text()
            f.write_text(ft[:ft.rindex("}")] + "    left { type cyclic; }\n    right { type cyclic; }\n}\n")
    return dst


def write(dst, text):
    (dst / "constant/couplingProperties").write_text(HEADER + text)


def flow_of(prod, dst, solver):
    fc = prod.GeneralFoamCase(dst, solver)
    f = fc.ldu_case.flow_control
    out = dict(on=f.on, ubar=tuple(f.ubar), relaxation=f.relaxation, gradient0=f.gradient0, superficial=f.superficial)
    fc.close()
    return out


def test_the_sub_dictionary_maps_to_the_descriptor(prod, tmp_path):
    pim, ico = general_copy(tmp_path, "bed_pimple"), general_copy(tmp_path, "cavity_ico")
    P, I = prod.FY_SOLVER_PIMPLE, prod.FY_SOLVER_ICO
    off = dict(on=0, ubar=(0.0, 0.0, 0.0), relaxation=0.0, gradient0=0.0, superficial=0)
    assert flow_of(prod, pim, P) == off and flow_of(prod, ico, I) == off              # an absent file reads as zero
    assert prod.LduCase().flow_control.on == 0
    write(pim, "dragModel Beetstra;\n")
    assert flow_of(prod, pim, P) == off                                                # ... and so does a file without the entry
    write(pim, "meanVelocityForce { Ubar (0.1335 0 0); relaxation 1.0; superficial off; }\n")
    assert flow_of(prod, pim, P) == dict(on=1, ubar=(0.1335, 0.0, 0.0), relaxation=1.0, gradient0=0.0, superficial=0)
    write(pim, "meanVelocityForce\n{\n    selectionMode all;\n    fields (U.water);\n    Ubar (0.03 0 -0.04);\n    relaxation 0.25;\n    superficial on;\n    active on;\n}\n")
    assert flow_of(prod, pim, P) == dict(on=1, ubar=(0.03, 0.0, -0.04), relaxation=0.25, gradient0=0.0, superficial=1)
    write(pim, "meanVelocityForce { Ubar (1 0 0); }\n")
    assert flow_of(prod, pim, P) == dict(on=1, ubar=(1.0, 0.0, 0.0), relaxation=1.0, gradient0=0.0, superficial=0)      # OpenFOAM's default relaxation
    write(pim, "meanVelocityForce { Ubar (1 0 0); active off; bogus 3; }\n")
    with pytest.raises(prod.FoamYadeError, match="bogus"):                             # (entries are checked whether active or not)
        flow_of(prod, pim, P)
    write(pim, "meanVelocityForce { Ubar (1 0 0); relaxation 0.5; active off; }\n")
    assert flow_of(prod, pim, P) == off                                                # active off reads as off
    write(ico, "meanVelocityForce { Ubar (0 0.2 0); relaxation 0.5; fields (U); selectionMode all; superficial off; }\n")
    assert flow_of(prod, ico, I) == dict(on=1, ubar=(0.0, 0.2, 0.0), relaxation=0.5, gradient0=0.0, superficial=0)
    # a general mesh without a cyclic pair takes it too
    walls = general_copy(tmp_path / "w", "cavity_ico", periodic=False)
    write(walls, "meanVelocityForce { Ubar (0.1 0 0); }\n")
    assert flow_of(prod, walls, I)["on"] == 1


@pytest.mark.parametrize("name,body,entry,accepted", [
    ("bed_pimple", "Ubar (1 0 0); gradient 3;", "meanVelocityForce.gradient", ["Ubar", "relaxation", "superficial", "selectionMode", "fields", "active"]),
    ("bed_pimple", "Ubar (1 0 0); cellZone inlet;", "meanVelocityForce.cellZone", ["Ubar", "relaxation", "superficial", "selectionMode", "fields", "active"]),
    ("bed_pimple", "Ubar (1 0 0); selectionMode cellZone;", "meanVelocityForce.selectionMode", ["all"]),
    ("bed_pimple", "Ubar (1 0 0); fields (U);", "meanVelocityForce.fields", ["(U.water)"]),
    ("cavity_ico", "Ubar (1 0 0); fields (U.water);", "meanVelocityForce.fields", ["(U)"]),
    ("cavity_ico", "Ubar (1 0 0); fields (U p);", "meanVelocityForce.fields", ["(U)"]),
    ("bed_pimple", "relaxation 1;", "meanVelocityForce.Ubar", ["(Ux Uy Uz)"]),
    ("bed_pimple", "Ubar (0 0 0);", "meanVelocityForce.Ubar", ["not zero"]),
    ("bed_pimple", "Ubar (1 0 0); relaxation 1.5;", "meanVelocityForce.relaxation", ["[0, 1]"]),
    ("bed_pimple", "Ubar (1 0 0); superficial maybe;", "meanVelocityForce.superficial", ["on", "off"]),
    ("cavity_ico", "Ubar (1 0 0); superficial on;", "meanVelocityForce.superficial", ["icoFoamYade", "off"]),
    ("bed_pimple", "Ubar (1 0 0); active perhaps;", "meanVelocityForce.active", ["on", "off"]),
])
def test_unknown_and_unsupported_entries_are_refused_by_name(prod, tmp_path, name, body, entry, accepted):
    dst = general_copy(tmp_path, name)
    write(dst, "meanVelocityForce { %s }\n" % body)
    with pytest.raises(prod.FoamYadeError) as e:
        flow_of(prod, dst, prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO)
    msg = str(e.value)
    assert "error 5" in msg and "constant/couplingProperties" in msg and entry in msg, msg      # FY_ERR_UNSUPPORTED
    for w in accepted:
        assert w in msg, (w, msg)


def test_a_block_case_is_refused_and_fvOptions_is_not_read(prod, tmp_path):
    dst = tmp_path / "bed_pimple"
    shutil.copytree(os.path.join(CASES, "bed_pimple"), dst)
    write(dst, "meanVelocityForce { Ubar (0.1 0 0); }\n")
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert "error 5" in str(e.value) and "meanVelocityForce" in str(e.value) and "needs a general mesh: the block has no periodic sides" in str(e.value)
    write(dst, "meanVelocityForce { Ubar (0.1 0 0); active off; }\n")
    prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE).close()
    gen = general_copy(tmp_path / "g", "bed_pimple")
    (gen / "constant/fvOptions").write_text("momentumSource { type meanVelocityForce; this is ( not even a dictionary\n")
    assert flow_of(prod, gen, prod.FY_SOLVER_PIMPLE)["on"] == 0                        # the reference's solvers carry no fvOptions: the file is not opened


def test_gradient0_comes_from_the_start_time_directory(prod, tmp_path):
    dst = general_copy(tmp_path, "bed_pimple")
    write(dst, "meanVelocityForce { Ubar (0.05 0 0); }\n")
    os.makedirs(dst / "0/uniform")
    (dst / "0/uniform/meanVelocityForceProperties").write_text("FoamFile { version 2.0; format ascii; class dictionary; object meanVelocityForceProperties; }\ngradient 0.12345678901234568;\n")
    assert flow_of(prod, dst, prod.FY_SOLVER_PIMPLE)["gradient0"] == 0.12345678901234568
    (dst / "0/uniform/meanVelocityForceProperties").write_text("FoamFile { version 2.0; format ascii; class dictionary; object meanVelocityForceProperties; }\ngradiant 1;\n")
    with pytest.raises(prod.FoamYadeError, match="meanVelocityForceProperties"):
        flow_of(prod, dst, prod.FY_SOLVER_PIMPLE)


@pytest.mark.gpu
def test_foamYadeHip_holds_the_flow_rate_and_restarts_from_its_gradient(prod, tmp_path):
    """foamYadeHip on a periodic general copy of bed_pimple: the restart file in each written time, OpenFOAM's line once per step, and a second run from the latest
    time that begins with that file's gradient"""
    dst = general_copy(tmp_path, "bed_pimple")
    write(dst, "meanVelocityForce { Ubar (0.05 0 0); relaxation 0.8; }\n")
    exe = os.path.join(os.path.dirname(prod.__file__), "bin", "foamYadeHip")
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = re.findall(r"^Pressure gradient source: uncorrected Ubar = (\S+), pressure gradient = (\S+)$", out.stdout, flags=re.M)
    assert len(lines) == 10 == out.stdout.count("\nTime = ")                            # endTime 0.002 / deltaT 0.0002: once per step
    assert "meanVelocityForce: Ubar (0.05 0 0), relaxation 0.8, superficial off, initial pressure gradient = 0\n" in out.stdout
    grads = {}
    for t in ("0.001", "0.002"):
        f = dst / t / "uniform/meanVelocityForceProperties"
        assert f.exists(), t
        grads[t] = float(re.search(r"^gradient\s+(\S+);", f.read_text(), flags=re.M).group(1))
    assert grads["0.001"] == float(lines[4][1]) and grads["0.002"] == float(lines[9][1]) and grads["0.002"] != 0.0      # 17 digits: the very number
    assert float(lines[9][0]) == pytest.approx(0.05, rel=0.3)                           # (the uncorrected bulk velocity nears Ubar)
    cd = (dst / "system/controlDict").read_text()
    cd = re.sub(r"startFrom\s+\w+;", "startFrom       latestTime;", cd)
    cd = re.sub(r"endTime\s+[0-9.eE+-]+;", "endTime         0.003;", cd)
    (dst / "system/controlDict").write_text(cd)
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.ldu_case.flow_control.gradient0 == grads["0.002"]
    s = prod.LduSolver.from_foam_case(fc)
    assert s.flow_control() == dict(gradient=grads["0.002"], ubar=0.0, rAU_ave=0.0, dGradP=0.0, corrections=0)
    s.step()
    f = s.flow_control()                                                                # the first assembly used it: gradP0 = gradient0 + 0, whatever dGradP became
    assert abs((f["gradient"] - f["dGradP"]) - grads["0.002"]) <= 2 * np.spacing(abs(f["gradient"]) + abs(f["dGradP"])) and f["corrections"] > 0
    s.close(); fc.close()
    out2 = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out2.returncode == 0, out2.stdout[-2000:] + out2.stderr[-2000:]
    assert "initial pressure gradient = %.17g\n" % grads["0.002"] in out2.stdout
    assert out2.stdout.count("Pressure gradient source:") == 5 and (dst / "0.003/uniform/meanVelocityForceProperties").exists()
