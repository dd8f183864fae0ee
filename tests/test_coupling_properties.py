"""constant/couplingProperties: the drag closure and the opt-in force models of a case directory (dragModel, liftModel, addedMass, gaussianTorque), read by one
function for block and general cases and carried in fy_case_desc / fy_ldu_case (zero = the reference's behaviour).  Copies of tests/golden/cases."""
import os
import shutil

import numpy as np
import pytest

import poly_meshes as pm

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "cases")
HEADER = "FoamFile { version 2.0; format ascii; class dictionary; location \"constant\"; object couplingProperties; }\n"
KINDS = ["block", "general"]


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def case_copy(tmp_path, name, kind):
    dst = tmp_path / name
    shutil.copytree(os.path.join(CASES, name), dst)
    if kind == "general":                    # the same box and patches as a polyhedral mesh (no blockMeshDict: nothing but constant/polyMesh describes it)
        os.remove(dst / "system/blockMeshDict")
        if name == "cavity_ico":
            pm.write_poly_mesh_files(dst, pm.hex_block(4, 4, 4, (0.1, 0.1, 0.1), pm.shear(0.2, 0.1, 0.1), patches=[("movingWall", [3]), ("fixedWalls", [0, 1, 2, 4, 5])]))
        else:
            mesh = pm.hex_block(4, 4, 8, (0.06, 0.06, 0.12), lambda P: P + np.array([-0.03, -0.03, 0.0]), patches=[("bottom", [4]), ("top", [5]), ("walls", [0, 1, 2, 3])])
            pm.write_poly_mesh_files(dst, mesh, {"bottom": "patch", "top": "patch", "walls": "wall"})
    return dst


def read(prod, dst, solver, kind):
    """(drag_law, force_models) as the descriptor a solver would be made from carries them"""
    if kind == "general":
        fc = prod.GeneralFoamCase(dst, solver)
        out = (fc.ldu_case.drag_law, fc.ldu_case.force_models)
    else:
        fc = prod.FoamCase(dst, solver)
        out = (fc.case.drag_law, fc.case.force_models)
    fc.close()
    return out


def write(dst, text):
    (dst / "constant/couplingProperties").write_text(HEADER + text)


@pytest.mark.parametrize("kind", KINDS)
def test_no_file_means_the_reference_behaviour(prod, tmp_path, kind):
    assert read(prod, case_copy(tmp_path, "bed_pimple", kind), prod.FY_SOLVER_PIMPLE, kind) == (prod.DRAG_REFERENCE, 0)
    assert read(prod, case_copy(tmp_path, "cavity_ico", kind), prod.FY_SOLVER_ICO, kind) == (prod.DRAG_REFERENCE, 0)
    assert prod.case_defaults(prod.FY_SOLVER_PIMPLE).drag_law == 0 and prod.case_defaults(prod.FY_SOLVER_PIMPLE).force_models == 0
    assert prod.CaseDesc().drag_law == 0 and prod.LduCase().force_models == 0              # a zero-initialised descriptor is the reference's behaviour


@pytest.mark.parametrize("kind", KINDS)
def test_each_word_maps_to_its_constant(prod, tmp_path, kind):
    dst = case_copy(tmp_path, "bed_pimple", kind)
    P = prod.FY_SOLVER_PIMPLE
    for word, law in (("reference", prod.DRAG_REFERENCE), ("DiFelice", prod.DRAG_DI_FELICE), ("KochHill", prod.DRAG_KOCH_HILL), ("Beetstra", prod.DRAG_BEETSTRA)):
        write(dst, f"dragModel {word};\n")
        assert read(prod, dst, P, kind) == (law, 0)
        assert prod.DRAG_LAWS[word] == law
    write(dst, "liftModel SaffmanMei;\n")
    assert read(prod, dst, P, kind) == (0, prod.FORCE_SAFFMAN_MEI_LIFT)
    write(dst, "liftModel none;\naddedMass on;\n")
    assert read(prod, dst, P, kind) == (0, prod.FORCE_ADDED_MASS)
    write(dst, "gaussianTorque on;\naddedMass off;\n")
    assert read(prod, dst, P, kind) == (0, prod.FORCE_GAUSSIAN_TORQUE)
    write(dst, "dragModel Beetstra;\nliftModel SaffmanMei;\naddedMass on;\ngaussianTorque on; // everything\n")
    assert read(prod, dst, P, kind) == (prod.DRAG_BEETSTRA, 7)
    write(dst, "// an empty dictionary\n")
    assert read(prod, dst, P, kind) == (0, 0)
    ico = case_copy(tmp_path, "cavity_ico", kind)
    write(ico, "dragModel SchillerNaumann;\nliftModel none;\naddedMass off;\ngaussianTorque off;\n")
    assert read(prod, ico, prod.FY_SOLVER_ICO, kind) == (prod.DRAG_SCHILLER_NAUMANN, 0)
    assert (prod.DRAG_SCHILLER_NAUMANN, prod.DRAG_LAWS["SchillerNaumann"]) == (4, 4)
    write(ico, "dragModel reference;\n")
    assert read(prod, ico, prod.FY_SOLVER_ICO, kind) == (0, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,text,entry,accepted", [
    ("bed_pimple", "dragModel Gidaspow;", "dragModel", ["reference", "DiFelice", "KochHill", "Beetstra"]),
    ("bed_pimple", "dragModel SchillerNaumann;", "dragModel", ["reference", "DiFelice", "KochHill", "Beetstra"]),
    ("cavity_ico", "dragModel Beetstra;", "dragModel", ["reference", "SchillerNaumann"]),
    ("cavity_ico", "dragModel WenYu;", "dragModel", ["reference", "SchillerNaumann"]),
    ("bed_pimple", "liftModel Saffman;", "liftModel", ["none", "SaffmanMei"]),
    ("cavity_ico", "liftModel SaffmanMei;", "liftModel", ["none"]),
    ("bed_pimple", "addedMass maybe;", "addedMass", ["on", "off"]),
    ("cavity_ico", "addedMass on;", "addedMass", ["off"]),
    ("cavity_ico", "gaussianTorque on;", "gaussianTorque", ["off"]),
])
def test_words_the_solver_cannot_take_are_refused_by_name(prod, tmp_path, kind, name, text, entry, accepted):
    dst = case_copy(tmp_path, name, kind)
    write(dst, text + "\n")
    with pytest.raises(prod.FoamYadeError) as e:
        read(prod, dst, prod.FY_SOLVER_PIMPLE if name == "bed_pimple" else prod.FY_SOLVER_ICO, kind)
    msg = str(e.value)
    assert "constant/couplingProperties" in msg and entry in msg
    for w in accepted:
        assert w in msg, (w, msg)
