"""Open boundaries from a case directory (general meshes only): inletOutlet for U, k and epsilon, pressureInletOutletVelocity for U -- what the reader accepts and
hands to fy_foam_case_ldu_desc, what it refuses by name, that a block keeps refusing the words, the round trip through a written time directory; on the GPU the run
from the directory against the hand-built solver, and the time directory a solver writes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import foam_dict_reader as fdr
from test_foam_case import CASES
from test_case_boundary_io import kepsilon_block
from test_ldu_case import cyclic_case
from test_ldu_wall_functions import wf_bed

UNSUPPORTED = 5                  # FY_ERR_UNSUPPORTED


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def edit(path, old, new):
    t = path.read_text()
    assert old in t, (path, old)
    path.write_text(t.replace(old, new, 1))


U_IO = "type inletOutlet; phi phi.water; inletValue uniform (0.001 0 -0.02); value uniform (0 0 0);"
U_PIO = "type pressureInletOutletVelocity; phi phi; value uniform (0 0 0);"
K_IO = "type inletOutlet; inletValue uniform 4e-4;"
EPS_IO = "type inletOutlet; phi phi.water; inletValue uniform 3e-3; value uniform 2e-3;"


def open_bed(tmp_path, u_top=U_PIO, k_top=K_IO, eps_top=EPS_IO, types=None):
    """the wavy general bed with RAS kEpsilon (bottom, top: patch; walls: wall + wall functions), its top open"""
    dst, mesh = wf_bed(tmp_path, types=types)
    edit(dst / "0/U.water", "top    { type zeroGradient; }", "top    { %s }" % u_top)
    edit(dst / "0/k.water", "top { type zeroGradient; }", "top { %s }" % k_top)
    edit(dst / "0/epsilon.water", "top { type zeroGradient; }", "top { %s }" % eps_top)
    return dst, mesh


def conditions(fc):
    lc, n = fc.ldu_case, len(fc.patch_names)
    return dict(U=(fc.u_bc, fc.u_value.tolist()), k=([lc.k_bc[q] for q in range(n)], [lc.k_value[q] for q in range(n)]),
                eps=([lc.eps_bc[q] for q in range(n)], [lc.eps_value[q] for q in range(n)]), nut=[lc.nut_bc[q] for q in range(n)])


@pytest.mark.parametrize("u_top", [U_IO, U_PIO])
def test_a_general_case_with_an_open_top_is_read(prod, tmp_path, u_top):
    dst, _ = open_bed(tmp_path, u_top=u_top)
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    top = fc.patch_names.index("top")
    c = conditions(fc)
    if u_top is U_IO:
        assert c["U"][0][top] == prod.FY_BC_U_INLET_OUTLET == 3 and c["U"][1][top] == [0.001, 0.0, -0.02]
    else:
        assert c["U"][0][top] == prod.FY_BC_U_PRESSURE_INLET_OUTLET == 4 and c["U"][1][top] == [0.0, 0.0, 0.0]
    assert c["k"][0][top] == prod.FY_BC_NUT_INLET_OUTLET == 4 and c["k"][1][top] == 4e-4
    assert c["eps"][0][top] == prod.FY_BC_NUT_INLET_OUTLET and c["eps"][1][top] == 3e-3
    assert c["nut"][top] == 0                                       # nut on such a patch takes what it takes today
    assert [b for q, b in enumerate(c["U"][0]) if q != top] == [prod.FY_BC_U_FIXED_VALUE] * 2
    # a time directory written from host arrays holds the entries; opened from it the case has the same description
    n = fc.field_cells
    rs = np.random.RandomState(3)
    fc.write_fields("0.5", rs.standard_normal((n, 3)), rs.standard_normal(n), alpha=np.ones(n), nut=rs.uniform(1e-6, 1e-5, n), k=rs.uniform(1e-4, 1e-3, n), epsilon=rs.uniform(1e-3, 1e-2, n))
    bf = lambda name: fdr.parse_file(os.path.join(str(dst), "0.5", name))["boundaryField"]["top"]
    u = bf("U.water")
    assert u["type"] == ("inletOutlet" if u_top is U_IO else "pressureInletOutletVelocity")
    if u_top is U_IO:
        assert u["inletValue"] == ["uniform", [0.001, 0, -0.02]] and u["phi"] == "phi.water"
    k, e = bf("k.water"), bf("epsilon.water")
    assert k["type"] == "inletOutlet" and k["inletValue"] == ["uniform", 4e-4] and k["value"] == ["uniform", 4e-4]      # (no value in the file: the inlet value is added)
    assert e["type"] == "inletOutlet" and e["inletValue"] == ["uniform", 3e-3] and e["value"] == ["uniform", 2e-3]      # (as read)
    fc.close()
    cd = dst / "system/controlDict"
    cd.write_text(re.sub(r"startFrom\s+\w+;", "startFrom latestTime;", cd.read_text()))
    again = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert again.start_name == "0.5" and conditions(again) == c
    again.close()


@pytest.mark.parametrize("field,entry,needles", [
    ("U.water", "type pressureInletOutletVelocity; tangentialVelocity uniform (1 0 0);", ["top", "tangentialVelocity"]),
    ("U.water", "type pressureInletOutletVelocity; phi phi.air;", ["top", "phi.air"]),
    ("U.water", "type inletOutlet; phi rhoPhi; inletValue uniform (0 0 0);", ["top", "rhoPhi"]),
    ("U.water", "type inletOutlet;", ["top", "inletValue uniform (x y z)"]),
    ("U.water", "type inletOutlet; inletValue nonuniform List<vector> 1((0 0 0));", ["top", "inletValue uniform (x y z)"]),
    ("k.water", "type inletOutlet; value uniform 1e-4;", ["top", "inletValue uniform <k>"]),
    ("epsilon.water", "type inletOutlet; phi phiv; inletValue uniform 1e-3;", ["top", "phiv"]),
])
def test_each_refusal_is_raised_by_name(prod, tmp_path, field, entry, needles):
    kw = {"U.water": "u_top", "k.water": "k_top", "epsilon.water": "eps_top"}[field]
    dst, _ = open_bed(tmp_path, **{kw: entry})
    with pytest.raises(prod.FoamYadeError) as e:
        prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    msg = str(e.value)
    assert msg.startswith("libfoamyade_hip error %d: " % UNSUPPORTED) and field in msg and all(w in msg for w in needles), msg


@pytest.mark.parametrize("cls", ["wall", "symmetryPlane", "symmetry"])
@pytest.mark.parametrize("field,entry", [("U.water", U_IO), ("U.water", U_PIO), ("k.water", K_IO), ("epsilon.water", EPS_IO)])
def test_an_open_condition_on_a_wall_or_symmetry_patch_is_refused_by_name(prod, tmp_path, cls, field, entry):
    kw = {"U.water": "u_top", "k.water": "k_top", "epsilon.water": "eps_top"}[field]
    args = dict(u_top="type %s;" % cls if cls != "wall" else "type noSlip;", k_top="type zeroGradient;", eps_top="type zeroGradient;")
    args[kw] = entry
    dst, _ = open_bed(tmp_path, types={"bottom": "patch", "top": cls, "walls": "wall"}, **args)
    if cls != "wall":
        edit(dst / "0/p", "top    { type fixedValue; value uniform 0; }", "top    { type %s; }" % cls)
    with pytest.raises(prod.FoamYadeError) as e:
        prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    msg = str(e.value)
    ty = entry.split(";")[0].split()[1]
    assert field in msg and "patch 'top'" in msg and ("%s on a %s patch is not supported" % (ty, cls)) in msg, msg


def test_an_open_condition_on_a_cyclic_patch_is_refused_by_name(prod, tmp_path):
    _, dst = cyclic_case(tmp_path)
    edit(dst / "0/U", "left { type cyclic; }", "left { type inletOutlet; inletValue uniform (0 0 0); }")
    with pytest.raises(prod.FoamYadeError) as e:
        prod.GeneralFoamCase(dst)
    assert "patch 'left'" in str(e.value) and "inletOutlet on a cyclic patch is not supported" in str(e.value), str(e.value)


BLOCK_LISTS = {"velocity": "fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip", "k": "zeroGradient, kqRWallFunction, fixedValue",
               "epsilon": "zeroGradient, fixedValue, epsilonWallFunction"}


@pytest.mark.parametrize("field,entry,word", [("U.water", U_IO, "velocity"), ("U.water", U_PIO, "velocity"), ("k.water", K_IO, "k"), ("epsilon.water", EPS_IO, "epsilon")])
def test_a_block_case_with_the_same_entries_is_still_refused(prod, tmp_path, field, entry, word):
    """the four entry kinds on the block bed with RAS kEpsilon: each is refused with the block's own message and list, as before"""
    dst = kepsilon_block(tmp_path, wall_functions=False)
    edit(dst / "0" / field, "top    { type zeroGradient; }", "top    { %s }" % entry)
    ty = entry.split(";")[0].split()[1]
    with pytest.raises(prod.FoamYadeError) as e:
        prod.FoamCase(dst, prod.FY_SOLVER_PIMPLE)
    msg = str(e.value)
    assert field in msg and msg.endswith("patch 'top': %s boundary type '%s' is not supported (%s)" % (word, ty, BLOCK_LISTS[word])), msg


def test_the_unknown_type_message_of_a_general_mesh_keeps_its_list(prod, tmp_path):
    dst, _ = open_bed(tmp_path, u_top="type outletInlet; outletValue uniform (0 0 0);")
    with pytest.raises(prod.FoamYadeError) as e:
        prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert str(e.value).endswith("velocity boundary type 'outletInlet' is not supported on a general mesh (fixedValue, noSlip, zeroGradient, symmetryPlane, symmetry, slip)"), str(e.value)


# ---- on the device ---------------------------------------------------------------------------------------------------------------------------------------------------

def hand_built(prod, mesh, lc, fc):
    """the solver of the case's arrays and controls built by hand: every plain number of fy_ldu_case as read, the patch arrays spelled out"""
    n = len(fc.patch_names)
    plain = {nm: getattr(lc, nm) for nm, ty in prod.LduCase._fields_ if ty in (prod.C.c_double, prod.C.c_int32, prod.C.c_uint32) and nm not in ("dt", "nu", "solid_stats")}
    plain["g"] = tuple(lc.g)
    top = fc.patch_names.index("top")
    assert fc.patch_names == ["bottom", "top", "walls"] and top == 1
    return prod.LduSolver(mesh, lc.dt, lc.nu, [0, prod.FY_BC_U_PRESSURE_INLET_OUTLET, 0], [(0, 0, 0.02), (0, 0, 0), (0, 0, 0)], [2, 1, 2], [0.0, 0.0, 0.0],
                          nut_bc=[lc.nut_bc[q] for q in range(n)], nut_val=[lc.nut_value[q] for q in range(n)], k_bc=[1, prod.FY_BC_NUT_INLET_OUTLET, 0], k_val=[3e-4, 4e-4, 0.0],
                          eps_bc=[1, prod.FY_BC_NUT_INLET_OUTLET, prod.BC_WALL_FUNCTION], eps_val=[2e-3, 3e-3, 0.0], **plain)


@pytest.mark.gpu
def test_run_from_a_case_directory_with_an_open_top_equals_the_hand_built_solver(prod, tmp_path):
    """a general pimpleFoamYade case whose top is pressureInletOutletVelocity with inletOutlet for k and epsilon: the library-driven run from the directory equals the
    hand-built LduSolver bit for bit; foamYadeHip runs the directory to its end time and writes the same fields (to the files' precision) with the open entries, the
    velocity's with the faces' values; the written directory opens again with the same description"""
    dst, mesh = open_bed(tmp_path)
    fc = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    c0 = conditions(fc)
    s = prod.LduSolver.from_foam_case(fc)
    h = hand_built(prod, mesh, fc.ldu_case, fc)
    h.set("nut", fc.initial_nut()); h.set("k", fc.initial_k()); h.set("epsilon", fc.initial_epsilon())
    for _ in range(10):
        s.step(); h.step()
    for nm in ("U", "p", "phi", "k", "epsilon", "nut", "U_open_inflow", "U_boundary"):
        np.testing.assert_array_equal(s.get(nm), h.get(nm), err_msg=nm)
    assert s.open_boundary_stats() == h.open_boundary_stats()
    U, k = s.get("U").reshape(-1, 3), s.get("k")
    top = slice(int(mesh["patch_start"][1]) - len(mesh["neighbour"]), int(mesh["patch_start"][1]) - len(mesh["neighbour"]) + int(mesh["patch_size"][1]))
    ub = s.get("U_boundary")[top]
    s.close(); h.close(); fc.close()
    exe = os.path.join(os.path.dirname(prod.__file__), "bin", "foamYadeHip")
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.rstrip().endswith("End")
    e = fdr.parse_file(os.path.join(str(dst), "0.002", "U.water"))["boundaryField"]["top"]
    assert e["type"] == "pressureInletOutletVelocity" and e["value"][0] == "nonuniform"
    ke = fdr.parse_file(os.path.join(str(dst), "0.002", "k.water"))["boundaryField"]["top"]
    assert ke["type"] == "inletOutlet" and ke["inletValue"] == ["uniform", 4e-4] and ke["value"] == ["uniform", 4e-4]
    cd = dst / "system/controlDict"
    cd.write_text(re.sub(r"startFrom\s+\w+;", "startFrom latestTime;", cd.read_text()))
    again = prod.GeneralFoamCase(dst, prod.FY_SOLVER_PIMPLE)
    assert again.start_name == "0.002" and conditions(again) == c0
    U1, _ = again.initial_fields()
    np.testing.assert_allclose(U1, U, rtol=0, atol=1e-12 * np.abs(U).max())
    np.testing.assert_allclose(again.initial_k(), k, rtol=0, atol=1e-12 * np.abs(k).max())
    written = np.array(e["value"][-1], dtype=float).reshape(-1, 3) if not isinstance(e["value"][-1], np.ndarray) else e["value"][-1].reshape(-1, 3)
    np.testing.assert_allclose(written, ub, rtol=0, atol=1e-12 * max(np.abs(ub).max(), 1e-300))
    again.close()
