"""constant/couplingProperties porousZones { ... }: the porous zones of a case directory, block and general (one reader), as fy_foam_case_porous_zones hands them to the
setters.  Copies of tests/golden/cases; the general copy is made the way test_flow_control_case.py makes its own."""
import os
import shutil

import numpy as np
import pytest

import poly_meshes as pm

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "cases")
HEADER = "FoamFile { version 2.0; format ascii; class dictionary; location \"constant\"; object couplingProperties; }\n"
PLATE = "plate { type DarcyForchheimer; box (-0.03 -0.03 0.02) (0.03 0.03 0.05); d (0 0 4e6); f (0 0 250); }"
SIEVE = "sieve\n    {\n        type    DarcyForchheimer;\n        active  on;\n        box     (-0.03 -0.03 0.08) (0 0.03 0.1);\n        d       (1e5 2e5 3e5);\n        f       (1.5 2.5 3.5);\n    }"


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def case_copy(tmp_path, kind, name="bed_pimple"):
    dst = tmp_path / name
    shutil.copytree(os.path.join(CASES, name), dst)
    if kind == "general":
        os.remove(dst / "system/blockMeshDict")
        mesh = pm.hex_block(4, 4, 8, (0.06, 0.06, 0.12), lambda P: P + np.array([-0.03, -0.03, 0.0]), patches=[("bottom", [4]), ("top", [5]), ("walls", [0, 1, 2, 3])])
        pm.write_poly_mesh_files(dst, mesh, {"bottom": "patch", "top": "patch", "walls": "wall"})
    return dst


def write(dst, text):
    (dst / "constant/couplingProperties").write_text(HEADER + text)


def open_case(prod, dst, kind):
    return prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE) if kind == "block" else prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)


def zones_of(prod, dst, kind):
    fc = open_case(prod, dst, kind)
    z = fc.porous_zones()
    fc.close()
    return z


def centres(kind):
    """cell centres by solver cell label: bed_pimple's 12 x 12 x 24 block of 5 mm cells, or the 4 x 4 x 8 lattice of 15 mm cells of the general copy"""
    n, h = ((12, 12, 24), 0.005) if kind == "block" else ((4, 4, 8), 0.015)
    x = [o + (np.arange(m) + 0.5) * h for o, m in zip((-0.03, -0.03, 0.0), n)]
    K, J, I = np.meshgrid(x[2], x[1], x[0], indexing="ij")
    return np.stack([I.ravel(), J.ravel(), K.ravel()], axis=1)


@pytest.mark.parametrize("kind", ["block", "general"])
def test_the_sub_dictionary_maps_to_the_descriptor(prod, tmp_path, kind):
    dst = case_copy(tmp_path, kind)
    assert zones_of(prod, dst, kind) == []                                             # no file: no zones
    write(dst, "dragModel Beetstra;\n")
    assert zones_of(prod, dst, kind) == []                                             # a file without the sub-dictionary: no zones
    write(dst, "porousZones { }\n")
    assert zones_of(prod, dst, kind) == []
    write(dst, "dragModel Beetstra;\nporousZones\n{\n    %s\n    off { type DarcyForchheimer; box (-1 -1 -1) (1 1 1); d (1 1 1); f (0 0 0); active off; }\n    %s\n}\n" % (PLATE, SIEVE))
    z = zones_of(prod, dst, kind)
    assert [o["name"] for o in z] == ["plate", "sieve"]                                # file order; `active off` leaves a zone out (its box would overlap both)
    assert z[0]["d"] == (0.0, 0.0, 4e6) and z[0]["f"] == (0.0, 0.0, 250.0) and z[1]["d"] == (1e5, 2e5, 3e5) and z[1]["f"] == (1.5, 2.5, 3.5)
    C = centres(kind)
    want = [prod.cells_in_box(C, (-0.03, -0.03, 0.02), (0.03, 0.03, 0.05)), prod.cells_in_box(C, (-0.03, -0.03, 0.08), (0, 0.03, 0.1))]
    assert [w.size for w in want] == ([144 * 6, 72 * 4] if kind == "block" else [16 * 2, 8 * 2])
    for o, w in zip(z, want):
        assert o["cells"].dtype == np.int32 and np.array_equal(o["cells"], w), o["name"]


BAD = [
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 -1) (1 1 1); d (1 1 1); f (0 0 0); cellZone plate; } }", ["porousZones.a.cellZone", "type, box, d, f, active"]),
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 -1) (1 1 1); d (1 1 1); f (0 0 0); coordinateSystem { type cartesian; } } }", ["porousZones.a.coordinateSystem", "box"]),
    ("porousZones { a { type DarcyForchheimer; selectionMode all; d (1 1 1); f (0 0 0); } }", ["porousZones.a.selectionMode", "box"]),
    ("porousZones { a { type powerLaw; box (-1 -1 -1) (1 1 1); d (1 1 1); f (0 0 0); } }", ["porousZones.a.type powerLaw", "DarcyForchheimer"]),
    ("porousZones { a { box (-1 -1 -1) (1 1 1); d (1 1 1); f (0 0 0); } }", ["porousZones.a.type", "DarcyForchheimer"]),
    ("porousZones { a { type DarcyForchheimer; box (1 1 1) (2 2 2); d (1 1 1); f (0 0 0); } }", ["porousZones.a.box", "selects no cell", "closed box"]),
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 -1); d (1 1 1); f (0 0 0); } }", ["porousZones.a.box", "(x0 y0 z0) (x1 y1 z1)"]),
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 0) (1 1 0.06); d (1 1 1); f (0 0 0); } b { type DarcyForchheimer; box (-1 -1 0.04) (1 1 0.1); d (1 1 1); f (0 0 0); } }",
     ["porousZones.a", "porousZones.b", "overlap"]),
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 -1) (1 1 1); d (1 -1 1); f (0 0 0); } }", ["porousZones.a.d", ">= 0"]),
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 -1) (1 1 1); d (1 1 1); } }", ["porousZones.a.f", "(x y z)"]),
    ("porousZones { a { type DarcyForchheimer; box (-1 -1 -1) (1 1 1); d (1 1 1); f (0 0 0); active perhaps; } }", ["porousZones.a.active", "on | off"]),
    ("porousZones ( a b );", ["porousZones", "dictionary"]),
]


@pytest.mark.parametrize("kind", ["block", "general"])
@pytest.mark.parametrize("text,words", BAD, ids=[b[1][0].split()[0] + str(q) for q, b in enumerate(BAD)])
def test_refusals_by_name(prod, tmp_path, kind, text, words):
    dst = case_copy(tmp_path, kind)
    write(dst, text + "\n")
    with pytest.raises(prod.FoamYadeError) as e:
        zones_of(prod, dst, kind)
    msg = str(e.value)
    assert "constant/couplingProperties" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_more_zones_than_the_solver_takes_and_a_decomposed_case(prod, tmp_path):
    dst = case_copy(tmp_path, "block")
    body = " ".join("z%d { type DarcyForchheimer; box (-1 -1 %g) (1 1 %g); d (1 1 1); f (0 0 0); }" % (q, 0.01 * q, 0.01 * q + 0.009) for q in range(9))
    write(dst, "porousZones { %s }\n" % body)
    with pytest.raises(prod.FoamYadeError) as e:
        zones_of(prod, dst, "block")
    assert "error 5" in str(e.value) and "FY_POROUS_MAX_ZONES" in str(e.value)
    write(dst, "porousZones { %s }\n" % PLATE)
    for r in range(2):
        (dst / f"processor{r}").mkdir()
        shutil.copytree(dst / "0", dst / f"processor{r}" / "0")
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE, processor=(0, 2))
    msg = str(e.value)
    assert "error 5" in msg and "porousZones.plate" in msg and "-parallel" in msg and "active off" in msg
    write(dst, "porousZones { %s }\n" % PLATE.replace("f (0 0 250);", "f (0 0 250); active off;"))
    prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE, processor=(0, 2)).close()               # ... and `active off` is accepted there
    (dst / "constant/fvOptions").write_text("porosity { type explicitPorositySource; this is ( not even a dictionary\n")
    assert zones_of(prod, dst, "block") == []                                          # the reference's solvers carry no fvOptions: the file is not opened
