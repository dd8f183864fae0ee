"""The boundary conditions of a case's field files (U, p, nut, k, epsilon), read and written back, on both kinds of case: a block (fy_foam_case_open,
the six sides of the box) and a general polyhedral mesh (fy_foam_case_open_general, one entry per patch).  A time written with every field must reopen with the
same conditions and list the same entries; and the rules in which the two readers differ are pinned one by one."""
import os
import re
import shutil

import numpy as np
import pytest

import foam_dict_reader as fdr
import poly_meshes as pm
from test_foam_case import CASES, NUT_FILE, decompose_case, les_case
from test_ldu_case import cyclic_case, general_bed, general_cavity
from test_ldu_wall_functions import wf_bed

XMIN, XMAX, YMIN, YMAX, ZMIN, ZMAX = range(6)
FIELDS = ("U", "p", "nut", "k", "epsilon")
INVALID, UNSUPPORTED = 1, 5                  # FY_ERR_INVALID, FY_ERR_UNSUPPORTED


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def kepsilon_block(tmp_path, wall_functions=True):
    """test_foam_case.test_ras_kepsilon_case_is_read's case: bed_pimple with RAS kEpsilon, its k / epsilon / nut files (wall functions on the walls)"""
    dst = les_case(tmp_path)
    (dst / "constant/turbulenceProperties.water").write_text("simulationType RAS;\nRAS { RASModel kEpsilon; turbulence on; }\n")
    kfile = NUT_FILE.replace("object nut.water", "object k.water").replace("[0 2 -1 0 0 0 0]", "[0 2 -2 0 0 0 0]").replace("uniform 2e-6", "uniform 3e-4")
    efile = NUT_FILE.replace("object nut.water", "object epsilon.water").replace("[0 2 -1 0 0 0 0]", "[0 2 -3 0 0 0 0]").replace("uniform 2e-6", "uniform 5e-3").replace("uniform 1e-6", "uniform 4e-3")
    nfile = NUT_FILE
    if wall_functions:
        efile = efile.replace("walls  { type zeroGradient; }", "walls  { type epsilonWallFunction; value uniform 5e-3; }")
        nfile = nfile.replace("walls  { type zeroGradient; }", "walls  { type nutkWallFunction; kappa 0.4; E 9.0; value uniform 0; }").replace(
            "top    { type zeroGradient; }", "top    { type calculated; value uniform 3e-6; }")
        kfile = kfile.replace("walls  { type zeroGradient; }", "walls  { type kqRWallFunction; value uniform 3e-4; }")
    (dst / "0/k.water").write_text(kfile)
    (dst / "0/epsilon.water").write_text(efile)
    (dst / "0/nut.water").write_text(nfile)
    return dst


def symmetry_case(tmp_path):
    """test_ldu_case.test_general_case_with_symmetry_patches_is_read's case: a sheared cavity with a symmetryPlane and a symmetry patch"""
    mesh = pm.hex_block(5, 4, 3, (0.1, 0.1, 0.1), pm.shear(0.2, 0.0, 0.1), patches=[("movingWall", [3]), ("fixedWalls", [1, 2, 5]), ("mirror", [0]), ("mirror2", [4])])
    dst = general_cavity(tmp_path, mesh)
    b = dst / "constant/polyMesh/boundary"
    t = b.read_text()
    i, j = t.index("mirror"), t.index("mirror2")
    b.write_text(t[:i] + re.sub(r"type(\s+)wall", r"type\1symmetryPlane", t[i:j], count=1) + re.sub(r"type(\s+)wall", r"type\1symmetry", t[j:], count=1))
    for nm in ("U", "p"):
        ft = (dst / "0" / nm).read_text()
        k = ft.rindex("}")
        (dst / "0" / nm).write_text(ft[:k] + "    mirror { type symmetryPlane; }\n    mirror2 { type symmetry; }\n}\n")
    return dst


def field_files(fc):
    """the case's field file names, those of the fields it reads"""
    names = {"U": fc.u_name, "p": "p", "nut": "nut." + fc.phase, "k": "k." + fc.phase, "epsilon": "epsilon." + fc.phase}
    return {f: names[f] for f in FIELDS if f in ("U", "p") or os.path.exists(os.path.join(fc.dir, fc.start_name, names[f]))}


def entries(path):
    """boundaryField of a field file: [(patch, type, value or None)] in the file's order"""
    bf = fdr.parse_file(path)["boundaryField"]
    return [(name, e["type"], e.get("value")) for name, e in bf.items()]


def block_conditions(c):
    out = {}
    for f, bc, val in (("U", "u_bc", "u_value"), ("p", "p_bc", "p_value"), ("nut", "nut_bc", "nut_value"), ("k", "k_bc", "k_value"), ("epsilon", "eps_bc", "eps_value")):
        out[f] = (list(getattr(c, bc)), [list(v) if f == "U" else v for v in getattr(c, val)])
    out["wf"] = (c.wf_kappa, c.wf_E)
    return out


def ldu_conditions(lc, n):
    out = {}
    for f, bc, val in (("U", "u_bc", "u_value"), ("p", "p_bc", "p_value"), ("nut", "nut_bc", "nut_value"), ("k", "k_bc", "k_value"), ("epsilon", "eps_bc", "eps_value")):
        b, v = getattr(lc, bc), getattr(lc, val)
        out[f] = None if not b else ([b[q] for q in range(n)], [v[q] for q in range(3 * n if f == "U" else n)])
    out["wf"] = (lc.wf_kappa, lc.wf_E)
    return out


class Opened:
    """one case (or processor directory) as the product opens it, with what a time directory is compared by"""

    def __init__(self, prod, dst, solver, general=False, processor=None):
        self.fc = prod.GeneralFoamCase(dst, solver) if general else prod.FoamCase(dst, solver, processor=processor)
        self.fc.dir = str(dst) if processor is None else os.path.join(str(dst), "processor%d" % processor[0])
        self.general = general
        self.conditions = ldu_conditions(self.fc.ldu_case, len(self.fc.patch_names)) if general else block_conditions(self.fc.case)


def round_trip(prod, dst, solver, general=False, processor=None, expect=FIELDS):
    """write every field at 0.5 from fixed arrays, reopen 0.5 as the start time: the same conditions, the same entries, the written values"""
    a = Opened(prod, dst, solver, general, processor)
    files = field_files(a.fc)
    assert tuple(files) == expect
    n = a.fc.field_cells
    rs = np.random.RandomState(3)
    arrays = dict(U=rs.standard_normal((n, 3)), p=rs.standard_normal(n), alpha=rs.uniform(0.5, 1.0, n), nut=rs.uniform(1e-6, 1e-5, n),
                  k=rs.uniform(1e-4, 1e-3, n), epsilon=rs.uniform(1e-3, 1e-2, n))
    a.fc.write_fields("0.5", **arrays)
    for f, name in files.items():
        start, written = entries(os.path.join(a.fc.dir, "0", name)), entries(os.path.join(a.fc.dir, "0.5", name))
        if general:       # (a boundaryField entry of a name that is no patch is not written back on a general mesh)
            start = [e for e in start if e[0] in a.fc.patch_names]
        assert written == start, f
    cd = dst / "system/controlDict"
    text = cd.read_text()
    cd.write_text(re.sub(r"startFrom\s+\w+;", "startFrom latestTime;", text))
    b = Opened(prod, dst, solver, general, processor)
    cd.write_text(text)
    assert b.fc.start_name == "0.5"
    assert b.conditions == a.conditions
    U, p = b.fc.initial_fields()
    np.testing.assert_array_equal(U, arrays["U"]); np.testing.assert_array_equal(p, arrays["p"])
    for f, get in (("nut", "initial_nut"), ("k", "initial_k"), ("epsilon", "initial_epsilon")):
        if f in files:
            np.testing.assert_array_equal(getattr(b.fc, get)(), arrays[f])
    a.fc.close(); b.fc.close()
    return a


# ---- round trips ------------------------------------------------------------------------------------------------------------------------------------------------

def test_block_cavity_round_trip(prod, tmp_path):
    dst = tmp_path / "cavity"
    shutil.copytree(os.path.join(CASES, "cavity_ico"), dst)
    round_trip(prod, dst, prod.FY_SOLVER_ICO, expect=("U", "p"))


def test_block_kepsilon_round_trip(prod, tmp_path):
    a = round_trip(prod, kepsilon_block(tmp_path), prod.FY_SOLVER_PIMPLE)
    assert a.conditions["nut"][0] == [2, 2, 2, 2, 1, 3] and a.conditions["epsilon"][0] == [2, 2, 2, 2, 1, 0] and a.conditions["wf"] == (0.4, 9.0)


@pytest.mark.parametrize("real_output", [False, True])
def test_decomposed_block_round_trip(prod, tmp_path, real_output):
    """every rank of a decomposed case: the processor patches are written back next to the case's own, alpha's with U's type and value 1"""
    if real_output:           # (decomposePar's empty `value` lists on the inlet: accepted for U and p only -- the laminar case)
        dst = tmp_path / "bed"
        shutil.copytree(os.path.join(CASES, "bed_pimple"), dst)
        expect = ("U", "p")
    else:
        dst = kepsilon_block(tmp_path)
        expect = FIELDS
    decompose_case(dst, 3, real_output=real_output)
    for r in range(3):
        a = round_trip(prod, dst, prod.FY_SOLVER_PIMPLE, processor=(r, 3), expect=expect)
        alpha = entries(os.path.join(a.fc.dir, "0.5", "alpha.water"))
        procs = [e for e in alpha if e[0].startswith("procBoundary")]
        assert [e[0] for e in alpha] == ["bottom", "top", "walls"] + [e[0] for e in procs] and len(procs) == (1 if r in (0, 2) else 2)
        assert all(e[1:] == ("processor", ["uniform", 1]) for e in procs)


def test_general_cyclic_round_trip(prod, tmp_path):
    _, dst = cyclic_case(tmp_path)
    a = round_trip(prod, dst, prod.FY_SOLVER_ICO, general=True, expect=("U", "p"))
    assert a.conditions["U"][0] == [0, 0, 1, 1] and a.conditions["p"][0] == [0, 0, 0, 0]


def test_general_symmetry_round_trip(prod, tmp_path):
    a = round_trip(prod, symmetry_case(tmp_path), prod.FY_SOLVER_ICO, general=True, expect=("U", "p"))
    assert a.conditions["U"][0] == [0, 0, 2, 2]


def test_general_wall_function_round_trip(prod, tmp_path):
    dst, _ = wf_bed(tmp_path)
    a = round_trip(prod, dst, prod.FY_SOLVER_PIMPLE, general=True)
    assert a.conditions["nut"][0] == [0, 0, 2] and a.conditions["epsilon"][0] == [1, 0, 2] and a.conditions["wf"] == (0.4, 9.0)


# ---- the rules in which the two readers differ ------------------------------------------------------------------------------------------------------------------

def edit(path, old, new):
    t = path.read_text()
    assert old in t, (path, old)
    path.write_text(t.replace(old, new, 1))


def refused(prod, open_case, rc, needle):
    with pytest.raises(prod.FoamYadeError) as e:
        open_case()
    msg = str(e.value)
    assert msg.startswith("libfoamyade_hip error %d: " % rc) and needle in msg, msg
    return msg


def block_bed(tmp_path):
    dst = tmp_path / "bed"
    shutil.copytree(os.path.join(CASES, "bed_pimple"), dst)
    return dst


def test_empty_patch_value_is_read_for_block_U_and_p_only(prod, tmp_path):
    """rule 1: `value nonuniform List<...> 0()` (a processor without a face of the patch) on a fixedValue U / p patch of a block; never for nut, nor on a general mesh"""
    dst = block_bed(tmp_path)
    edit(dst / "0/U.water", "value uniform (0 0 0.02);", "value nonuniform List<vector> 0();")
    edit(dst / "0/p", "top    { type fixedValue; value uniform 0; }", "top    { type fixedValue; value nonuniform List<scalar> 0(); }")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.case.u_bc[ZMIN] == 0 and list(fc.case.u_value[ZMIN]) == [0, 0, 0] and fc.case.p_bc[ZMAX] == 1 and fc.case.p_value[ZMAX] == 0
    fc.close()
    dst = kepsilon_block(tmp_path / "k")
    edit(dst / "0/nut.water", "value uniform 1e-6;", "value nonuniform List<scalar> 0();")
    refused(prod, lambda: prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "nut.water: patch 'bottom': fixedValue needs 'value uniform <nut>'")
    dst, _ = general_bed(tmp_path / "g")
    edit(dst / "0/U.water", "value uniform (0 0 0.02);", "value nonuniform List<vector> 0();")
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "U.water: patch 'bottom': fixedValue needs 'value uniform (x y z)'")
    dst, _ = general_bed(tmp_path / "g2")
    edit(dst / "0/p", "top    { type fixedValue; value uniform 0; }", "top    { type fixedValue; value nonuniform List<scalar> 0(); }")
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "/p: patch 'top': fixedValue needs 'value uniform <p>'")


def test_fixed_flux_pressure_with_either_solver_on_a_block_pimple_only_on_a_general_mesh(prod, tmp_path):
    """rule 2"""
    dst = tmp_path / "cavity"
    shutil.copytree(os.path.join(CASES, "cavity_ico"), dst)
    edit(dst / "0/p", "zeroGradient", "fixedFluxPressure")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    assert fc.case.p_bc[YMAX] == prod.FY_BC_P_FIXED_FLUX
    fc.close()
    dst, _ = general_bed(tmp_path)
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.p_bc == [2, 1, 2]
    fc.close()
    mesh = pm.hex_block(4, 4, 4, (0.1, 0.1, 0.1), pm.shear(0.2), patches=[("movingWall", [3]), ("fixedWalls", [0, 1, 2, 4, 5])])
    dst = general_cavity(tmp_path / "g", mesh)
    edit(dst / "0/p", "zeroGradient", "fixedFluxPressure")
    refused(prod, lambda: prod.GeneralFoamCase(dst), UNSUPPORTED, "/p: patch 'movingWall': pressure boundary type 'fixedFluxPressure' is not supported on a general mesh "
            "(zeroGradient, symmetryPlane, symmetry, fixedValue; fixedFluxPressure with pimpleFoamYade)")


def test_nut_calculated(prod, tmp_path):
    """rule 3: on a block `calculated` needs kEqn / kEpsilon; on a general mesh without a k equation it is a fixed value and needs `value uniform`"""
    dst = les_case(tmp_path)                  # Smagorinsky
    edit(dst / "0/nut.water", "top    { type zeroGradient; }", "top    { type calculated; value uniform 3e-6; }")
    refused(prod, lambda: prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "nut.water: patch 'top': nut boundary type 'calculated' is not supported "
            "(zeroGradient, fixedValue; calculated / nutkWallFunction with kEqn / kEpsilon)")
    dst, _ = wf_bed(tmp_path / "g", model="LES { LESModel Smagorinsky; delta cubeRootVol; turbulence on; cubeRootVolCoeffs { deltaCoeff 1; } }", nut_walls="calculated; value uniform 3e-6;")
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert [fc.ldu_case.nut_bc[q] for q in range(3)] == [0, 0, 1] and fc.ldu_case.nut_value[2] == 3e-6
    fc.close()
    dst, _ = wf_bed(tmp_path / "g2", model="LES { LESModel Smagorinsky; delta cubeRootVol; turbulence on; cubeRootVolCoeffs { deltaCoeff 1; } }", nut_walls="calculated;")
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "nut.water: patch 'walls': calculated needs 'value uniform <nut>'")
    dst, _ = wf_bed(tmp_path / "g3", nut_walls="calculated;")      # (kEpsilon: the value is optional)
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "epsilonWallFunction takes its constants")


def test_checks_made_on_a_general_mesh_only(prod, tmp_path):
    """rule 4: the wall-function patch class, the constraint type of an entry, cyclic entries"""
    dst = kepsilon_block(tmp_path)            # bottom is of type patch in blockMeshDict: a block takes a wall function there
    edit(dst / "0/nut.water", "bottom { type fixedValue; value uniform 1e-6; }", "bottom { type nutkWallFunction; value uniform 0; }")
    edit(dst / "0/epsilon.water", "bottom { type fixedValue; value uniform 4e-3; }", "bottom { type epsilonWallFunction; value uniform 0; }")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.case.nut_bc[ZMIN] == 2 and fc.case.eps_bc[ZMIN] == 2
    fc.close()
    dst, _ = wf_bed(tmp_path / "g", types={"bottom": "patch", "top": "patch", "walls": "patch"})
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "nut.water: patch 'walls': nutkWallFunction is a wall function, but the patch is of type 'patch' "
            "(constant/polyMesh/boundary), not wall")
    dst, _ = wf_bed(tmp_path / "g2", k_walls="kqRWallFunction; value uniform 3e-4;", types={"bottom": "patch", "top": "patch", "walls": "wall"})
    t = (dst / "0/k.water").read_text()
    (dst / "0/k.water").write_text(t.replace("top { type zeroGradient; }", "top { type kqRWallFunction; }"))
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)         # (k's wall function is not class-checked)
    assert [fc.ldu_case.k_bc[q] for q in range(3)] == [1, 0, 0]
    fc.close()
    dst = symmetry_case(tmp_path / "s")
    edit(dst / "0/p", "mirror2 { type symmetry; }", "mirror2 { type zeroGradient; }")
    refused(prod, lambda: prod.GeneralFoamCase(dst), INVALID, "/p: patch 'mirror2' is a symmetry patch (constant/polyMesh/boundary): its entry must be of that type, not 'zeroGradient'")
    dst, _ = wf_bed(tmp_path / "g3")
    for f in ("U.water", "p", "nut.water", "k.water", "epsilon.water"):
        t = (dst / "0" / f).read_text()
        (dst / "0" / f).write_text(re.sub(r"top \s*\{[^}]*\}", "top { type cyclic; }", t, count=1))
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)         # (a cyclic entry on a plain patch: zeroGradient)
    lc = fc.ldu_case
    assert (lc.u_bc[1], lc.p_bc[1], lc.nut_bc[1], lc.k_bc[1], lc.eps_bc[1]) == (1, 0, 0, 0, 0)
    fc.close()
    dst = block_bed(tmp_path / "b")
    edit(dst / "0/U.water", "top    { type zeroGradient; }", "top    { type cyclic; }")
    refused(prod, lambda: prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "U.water: patch 'top': velocity boundary type 'cyclic' is not supported "
            "(fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip)")


def test_wall_function_constants(prod, tmp_path):
    """rule 5: a general mesh defaults kappa / E per patch and refuses patches that differ; a block takes them as read, the last side's winning"""
    dst = kepsilon_block(tmp_path)
    edit(dst / "0/nut.water", "bottom { type fixedValue; value uniform 1e-6; }", "bottom { type nutkWallFunction; kappa 0.3; value uniform 0; }")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert (fc.case.wf_kappa, fc.case.wf_E) == (0.3, 9.0)          # (bottom = ZMIN comes after the walls; its E is not given)
    fc.close()
    dst, _ = wf_bed(tmp_path / "g", types={"bottom": "wall", "top": "patch", "walls": "wall"})
    edit(dst / "0/nut.water", "bottom { type zeroGradient; }", "bottom { type nutkWallFunction; value uniform 0; }")
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED,
            "nut.water: patches 'bottom' and 'walls' give nutkWallFunction different kappa / E: one set serves the case")


def test_epsilon_wall_function_needs_the_nut_wall_function_on_a_general_mesh_only(prod, tmp_path):
    """rule 6"""
    dst = kepsilon_block(tmp_path)
    edit(dst / "0/nut.water", "walls  { type nutkWallFunction; kappa 0.4; E 9.0; value uniform 0; }", "walls  { type zeroGradient; }")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert fc.case.eps_bc[XMIN] == 2 and fc.case.nut_bc[XMIN] == 0
    fc.close()
    dst, _ = wf_bed(tmp_path / "g", nut_walls="zeroGradient;")
    refused(prod, lambda: prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED,
            "epsilon.water: patch 'walls': epsilonWallFunction takes its constants from the patch's nut wall function, and nut.water is not nutkWallFunction there")


def test_entries_of_names_that_are_no_patch(prod, tmp_path):
    """rule 7: kept and written back on a block (with a value added where there was none), dropped on a general mesh"""
    dst = kepsilon_block(tmp_path)
    for f in ("U.water", "p", "nut.water", "k.water", "epsilon.water"):
        t = (dst / "0" / f).read_text()
        k = t.rindex("}")
        (dst / "0" / f).write_text(t[:k] + "    ghost { type zeroGradient; }\n    ghost2 { type fixedValue; value uniform %s; }\n}\n" % ("(1 2 3)" if f.startswith("U") else "7"))
    fc = prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    n = fc.field_cells
    fc.write_fields("0.5", np.zeros((n, 3)), np.zeros(n), np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n))
    fc.close()
    for f in ("U.water", "p", "nut.water", "k.water", "epsilon.water"):
        es = entries(dst / "0.5" / f)
        assert [e[0] for e in es] == ["bottom", "top", "walls", "ghost", "ghost2"]
        assert es[3][1:] == ("zeroGradient", ["uniform", [0, 0, 0]] if f.startswith("U") else ["uniform", 0])
        assert es[4][1:] == ("fixedValue", ["uniform", [1, 2, 3]] if f.startswith("U") else ["uniform", 7])
    assert [e[0] for e in entries(dst / "0.5/alpha.water")] == ["bottom", "top", "walls", "ghost", "ghost2"]
    dst, _ = wf_bed(tmp_path / "g")
    t = (dst / "0/p").read_text()
    (dst / "0/p").write_text(t[:t.rindex("}")] + "    ghost { type zeroGradient; }\n}\n")
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    n = fc.field_cells
    fc.write_fields("0.5", np.zeros((n, 3)), np.zeros(n), np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n))
    fc.close()
    assert [e[0] for e in entries(dst / "0.5/p")] == ["bottom", "top", "walls"]


BLOCK_LISTS = {"U": "velocity boundary type '%s' is not supported (fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip)",
               "p": "pressure boundary type '%s' is not supported (zeroGradient, fixedValue, fixedFluxPressure)",
               "nut": "nut boundary type '%s' is not supported (zeroGradient, fixedValue; calculated / nutkWallFunction with kEqn / kEpsilon)",
               "k": "k boundary type '%s' is not supported (zeroGradient, kqRWallFunction, fixedValue)",
               "epsilon": "epsilon boundary type '%s' is not supported (zeroGradient, fixedValue, epsilonWallFunction)"}
GENERAL_LISTS = {"U": "velocity boundary type '%s' is not supported on a general mesh (fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip)",
                 "p": "pressure boundary type '%s' is not supported on a general mesh (zeroGradient, symmetryPlane, symmetry, fixedValue; fixedFluxPressure with pimpleFoamYade)",
                 "nut": "nut boundary type '%s' is not supported on a general mesh (zeroGradient, symmetryPlane, symmetry, cyclic, fixedValue, calculated; "
                        "nutkWallFunction with kEqn / kEpsilon)",
                 "k": "k boundary type '%s' is not supported on a general mesh (zeroGradient, kqRWallFunction, symmetryPlane, symmetry, cyclic, fixedValue)",
                 "epsilon": "epsilon boundary type '%s' is not supported on a general mesh (zeroGradient, symmetryPlane, symmetry, cyclic, fixedValue, epsilonWallFunction)"}


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("field", FIELDS)
def test_unsupported_types_are_refused_with_each_kinds_message(prod, tmp_path, general, field):
    """rule 8: the type lists of the messages"""
    if general:
        dst, _ = wf_bed(tmp_path)
    else:
        dst = kepsilon_block(tmp_path)
    name = {"U": "U.water", "p": "p"}.get(field, field + ".water")
    t = (dst / "0" / name).read_text()
    (dst / "0" / name).write_text(re.sub(r"top \s*\{[^}]*\}", "top { type mixed; }", t, count=1))
    lists = GENERAL_LISTS if general else BLOCK_LISTS
    msg = refused(prod, lambda: (prod.GeneralFoamCase if general else prod.FoamCase)(dst, prod.FY_SOLVER_PIMPLE), UNSUPPORTED, "/0/%s: patch 'top': " % name)
    assert msg.endswith(lists[field] % "mixed"), msg
