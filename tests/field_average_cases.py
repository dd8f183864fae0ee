"""helpers of the fieldAverage tests: copies of tests/golden/cases as block or general cases, with a `functions` dictionary appended to controlDict"""
import os
import shutil

import numpy as np

import poly_meshes as pm

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "cases")
KINDS = ["block", "general"]
ON = "mean on; prime2Mean on; base time;"
MEAN = "mean on; prime2Mean off; base time;"


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


def add_functions(dst, body):
    with open(dst / "system/controlDict", "a") as f:
        f.write("\nfunctions\n{\n" + body + "\n}\n")


def field_average(fields, extra="", name="fieldAverage1"):
    """the text of one fieldAverage object: fields = [(file name, "mean ..; prime2Mean ..; base ..;")]"""
    items = "\n".join(f"            {nm} {{ {txt} }}" for nm, txt in fields)
    return f"    {name}\n    {{\n        type fieldAverage;\n        libs (\"libfieldFunctionObjects.so\");\n        {extra}\n        fields\n        (\n{items}\n        );\n    }}\n"


def open_case(prod, dst, solver, kind):
    return prod.GeneralFoamCase(dst, solver) if kind == "general" else prod.FoamCase(dst, solver)
