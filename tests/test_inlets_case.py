"""Inlets from a case directory (csrc/foam_case.cpp; DESIGN.md section 3 "Inlets"): the velocity entries `fixedValue` with
`value nonuniform List<vector>`, `uniformFixedValue` and `flowRateInletVelocity` become fy_case_desc.inlets / fy_ldu_case.inlets, start_time is the start directory's
time, and a written time directory keeps the entry's type and function dictionary with `value` as the faces' current values.  The CPU tests read and write case
directories; the GPU tests run them through foamYadeHip and restart them.  Meshes are written by tests/poly_meshes.py (there is no blockMesh here)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import inlets_ref as ir
import poly_meshes as pm

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "cases")
NX, NY, NZ = 6, 5, 7
LEN = (0.6, 0.5, 0.7)
ZMIN = 4
SINE = "uniformValue { type sine; amplitude 0.5; frequency 4; start 0.01; scale (0.01 0.02 0.3); level (0 0 0.4); }"
SINE_TERMS = [dict(f=dict(kind="sine", amplitude=0.5, frequency=4.0, t0=0.01), shape=(0.01, 0.02, 0.3)), dict(f=1.0, shape=(0.0, 0.0, 0.4))]


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


def vec_list(v):
    v = np.asarray(v, np.float64).reshape(-1, 3)
    return "nonuniform List<vector> %d\n(\n%s)\n" % (len(v), "".join("(%r %r %r)\n" % tuple(float(x) for x in r) for r in v))


def write_case(tmp_path, mesh, inlet_entry, name="case", end="0.015", write_interval=3, extra_control=""):
    """cavity_ico's dictionaries around `mesh` (one patch per side): inflow through zmin with the given entry, fixed pressure on zmax, walls elsewhere"""
    dst = tmp_path / name
    shutil.copytree(os.path.join(CASES, "cavity_ico"), dst)
    os.remove(dst / "system/blockMeshDict")
    pm.write_poly_mesh_files(dst, mesh, {"zmin": "patch", "zmax": "patch"})
    for nm in ("U", "p"):
        t = (dst / "0" / nm).read_text()
        body = "".join("    %s { type %s; }\n" % (s, "noSlip" if nm == "U" else "zeroGradient") for s in pm.SIDES)
        if nm == "U":
            body = body.replace("zmin { type noSlip; }", "zmin\n    {\n%s\n    }" % inlet_entry).replace("zmax { type noSlip; }", "zmax { type zeroGradient; }")
        else:
            body = body.replace("zmax { type zeroGradient; }", "zmax { type fixedValue; value uniform 0; }")
        (dst / "0" / nm).write_text(t[:t.index("boundaryField")] + "boundaryField\n{\n" + body + "}\n")
    cd = (dst / "system/controlDict").read_text()
    cd = re.sub(r"endTime\s+[0-9.eE+-]+;", "endTime         %s;" % end, cd)
    cd = re.sub(r"writeInterval\s+[0-9.eE+-]+;", "writeInterval   %d;" % write_interval, cd)
    (dst / "system/controlDict").write_text(cd + extra_control)
    return dst


def block_mesh(seed=4):
    """the 6 x 5 x 7 box as constant/polyMesh with its cells renumbered at random: neither the cells nor the boundary faces lie in the lattice's order"""
    return pm.hex_block(NX, NY, NZ, LEN, renumber_seed=seed)


def zmin_lattice_place(mesh):
    """for face q of patch zmin (the file's order): its place i + nx j on side z- ("U_boundary"'s order)"""
    s, n = int(mesh["patch_start"][ZMIN]), int(mesh["patch_size"][ZMIN])
    inv = np.argsort(mesh["perm"])                      # mesh cell -> lattice cell
    return inv[np.asarray(mesh["owner"])[s:s + n]] % (NX * NY)


def terms_of(prod, d, q=0):
    """inlet q of an InletsDesc as (patch, [(TimeFunction, shape_kind, shape pointer)])"""
    i = d.inlets[q]
    return i.patch, [(i.terms[m].f, i.terms[m].shape_kind, i.terms[m].shape) for m in range(i.n_terms)]


def eval_inlet(prod, d, n_faces, Sf, t, q=0):
    """the descriptor's inlet q at time t through fy_time_function_eval and the reference's shapes"""
    _, terms = terms_of(prod, d, q)
    out = np.zeros((n_faces, 3))
    for f, kind, sh in terms:
        a = prod.time_function_eval(f, t)
        if kind == prod.SHAPE_UNIFORM:
            S = np.tile([sh[0], sh[1], sh[2]], (n_faces, 1))
        elif kind == prod.SHAPE_PER_FACE:
            S = np.array([sh[q_] for q_ in range(3 * n_faces)]).reshape(n_faces, 3)
        else:
            S = ir.flow_rate_shape(Sf)
        out = out + a * S
    return out


# ------------------------------------------------------------------------------------------------ CPU: the reader
def test_block_nonuniform_list_is_placed_through_polyMesh(prod, tmp_path):
    """every boundary face of the list lands on its side at its lattice position, whatever the mesh's cell and face numbering"""
    mesh = block_mesh()
    n = NX * NY
    vals = np.random.RandomState(2).uniform(-1, 1, (n, 3))
    dst = write_case(tmp_path, mesh, "        type fixedValue;\n        value " + vec_list(vals) + ";")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    d = fc.case.inlets
    assert d.n == 1 and d.start_time == 0.0 and fc.case.u_bc[ZMIN] == prod.FY_BC_U_FIXED_VALUE
    patch, terms = terms_of(prod, d)
    assert patch == ZMIN and len(terms) == 1 and terms[0][1] == prod.SHAPE_PER_FACE and terms[0][0].kind == prod.TIME_CONSTANT and terms[0][0].value == 1.0
    got = np.array([terms[0][2][q] for q in range(3 * n)]).reshape(n, 3)
    want = np.zeros((n, 3)); want[zmin_lattice_place(mesh)] = vals
    assert np.array_equal(got, want)
    fc.close()


def test_block_with_blockMeshDict_alone_refuses_a_nonuniform_list(prod, tmp_path):
    dst = tmp_path / "cavity"
    shutil.copytree(os.path.join(CASES, "cavity_ico"), dst)
    t = (dst / "0/U").read_text().replace("value           uniform (1 0 0);", "value " + vec_list(np.ones((256, 3))) + ";")
    (dst / "0/U").write_text(t)
    with pytest.raises(prod.FoamYadeError, match="blockMeshDict alone"):
        prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    # ... while the function entries need no face order
    (dst / "0/U").write_text(t[:t.index("movingWall")] + "movingWall\n    {\n        type uniformFixedValue;\n        uniformValue constant (1 0 0);\n    }\n    fixedWalls { type noSlip; }\n}\n")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    patch, terms = terms_of(prod, fc.case.inlets)
    assert patch == 3 and [terms[0][2][q] for q in range(3)] == [1.0, 0.0, 0.0] and terms[0][0].kind == prod.TIME_CONSTANT
    fc.close()


ENTRIES = {
    "constant": ("type uniformFixedValue; uniformValue constant (0.1 0 0.3);", [dict(f=1.0, shape=(0.1, 0.0, 0.3))]),
    "bare_vector": ("type uniformFixedValue; uniformValue (0.1 0 0.3);", [dict(f=1.0, shape=(0.1, 0.0, 0.3))]),
    # a vector table: three terms, one scalar table per component with the shapes e_x, e_y, e_z
    "vector_table": ("type uniformFixedValue; uniformValue table ((0 (0 0 0.1)) (0.01 (0.02 0 0.3)) (0.05 (0 -0.01 0.2)));",
                     [dict(f=dict(kind="table", points=[(0, v0), (0.01, v1), (0.05, v2)]), shape=tuple(np.eye(3)[a])) for a, (v0, v1, v2) in enumerate(((0, 0.02, 0), (0, 0, -0.01), (0.1, 0.3, 0.2)))]),
    "table_repeat": ("type uniformFixedValue; uniformValue table ((0 (0 0 0.1)) (0.004 (0 0 0.3))); uniformValueCoeffs { outOfBounds repeat; }",
                     [dict(f=dict(kind="table", points=[(0, 0.0), (0.004, 0.0)], out_of_bounds="repeat"), shape=(1.0, 0, 0)),
                      dict(f=dict(kind="table", points=[(0, 0.0), (0.004, 0.0)], out_of_bounds="repeat"), shape=(0, 1.0, 0)),
                      dict(f=dict(kind="table", points=[(0, 0.1), (0.004, 0.3)], out_of_bounds="repeat"), shape=(0, 0, 1.0))]),
    "sine_dict": ("type uniformFixedValue; " + SINE, SINE_TERMS),
    "square_coeffs": ("type uniformFixedValue; uniformValue square; uniformValueCoeffs { amplitude 2; frequency 10; markSpace 3; scale (0 0 0.1); level (0 0 0.5); }",
                      [dict(f=dict(kind="square", amplitude=2.0, frequency=10.0, mark_space=3.0), shape=(0, 0, 0.1)), dict(f=1.0, shape=(0, 0, 0.5))]),
    "flow_constant": ("type flowRateInletVelocity; volumetricFlowRate 0.03; value uniform (0 0 0);", [dict(f=0.03, shape="flow_rate")]),
    "flow_table": ("type flowRateInletVelocity; volumetricFlowRate table ((0 0.01) (0.02 0.05));", [dict(f=dict(kind="table", points=[(0, 0.01), (0.02, 0.05)]), shape="flow_rate")]),
    "flow_sine": ("type flowRateInletVelocity; volumetricFlowRate { type sine; amplitude 1; frequency 5; scale 0.01; level 0.04; }",
                  [dict(f=dict(kind="sine", amplitude=0.01, frequency=5.0), shape="flow_rate"), dict(f=0.04, shape="flow_rate")]),
}


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_each_accepted_entry_round_trips_into_the_descriptor(prod, tmp_path, entry, general):
    """the descriptor's inlet evaluates, at several times, to what tests/inlets_ref.py makes of the same entry written as terms"""
    text, terms = ENTRIES[entry]
    mesh = pm.prism_block(3, 3, 2, LEN) if general else block_mesh()
    dst = write_case(tmp_path, mesh, "        " + text.replace("; ", ";\n        "))
    fc = prod.GeneralFoamCase(dst) if general else prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    d = (fc.ldu_case if general else fc.case).inlets
    assert d.n == 1 and d.inlets[0].patch == ZMIN and d.inlets[0].n_terms == len(terms)
    n = int(mesh["patch_size"][ZMIN]) if general else NX * NY
    Sf = np.tile([0.0, 0.0, -1.0], (n, 1)) * (LEN[0] * LEN[1] / n)          # (equal faces: the flow-rate shape needs only their ratio)
    for t in (0.0, 0.003, 0.01, 0.0137, 0.031, 0.26):
        got, want = eval_inlet(prod, d, n, Sf, t), ir.inlet_values(terms, t, Sf)
        assert np.abs(got - want).max() <= 1e-14 * max(np.abs(want).max(), 1e-300), (entry, t)
    fc.close()


def test_general_nonuniform_list_ascii_and_binary(prod, tmp_path):
    mesh = pm.prism_block(3, 3, 2, LEN)
    n = int(mesh["patch_size"][ZMIN])
    vals = np.random.RandomState(5).uniform(-1, 1, (n, 3))
    dst = write_case(tmp_path, mesh, "        type fixedValue;\n        value " + vec_list(vals) + ";")
    fc = prod.GeneralFoamCase(dst)
    _, terms = terms_of(prod, fc.ldu_case.inlets)
    assert terms[0][1] == prod.SHAPE_PER_FACE and np.array_equal(np.array([terms[0][2][q] for q in range(3 * n)]).reshape(n, 3), vals)
    fc.close()
    raw = (dst / "0/U").read_bytes()
    a, b = raw.index(b"nonuniform List<vector>", raw.index(b"zmin")), raw.index(b";", raw.index(b"zmin"))
    b = raw.index(b")\n;", a) + 3
    binary = raw[:a] + b"nonuniform List<vector> %d(" % n + vals.astype("<f8").tobytes() + b");" + raw[b:]
    binary = binary.replace(b"format      ascii;", b'format      binary;\n    arch        "LSB;label=32;scalar=64";')
    (dst / "0/U").write_bytes(binary)
    fc = prod.GeneralFoamCase(dst)
    _, terms = terms_of(prod, fc.ldu_case.inlets)
    assert np.array_equal(np.array([terms[0][2][q] for q in range(3 * n)]).reshape(n, 3), vals)
    fc.close()


@pytest.mark.parametrize("text,word", [
    ("type uniformFixedValue; uniformValue tableFile; uniformValueCoeffs { file \"x\"; }", "tableFile"),
    ("type uniformFixedValue; uniformValue polynomial ((1 0));", "polynomial"),
    ("type uniformFixedValue; uniformValue coded;", "coded"),
    ("type uniformFixedValue; uniformValue table ((0 (0 0 1)) (1 (0 0 2))); uniformValueCoeffs { outOfBounds error; }", "outOfBounds 'error'"),
    ("type uniformFixedValue; uniformValue table ((0 (0 0 1)) (1 (0 0 2))); uniformValueCoeffs { outOfBounds warn; }", "outOfBounds 'warn'"),
    ("type uniformFixedValue; uniformValue table ((0 (0 0 1)) (1 (0 0 2))); uniformValueCoeffs { interpolationScheme spline; }", "interpolationScheme"),
    ("type uniformFixedValue; uniformValue sine;", "coefficients"),
    ("type uniformFixedValue; uniformValue { type sine; amplitude 1; scale (0 0 1); level (0 0 0); }", "frequency"),
    ("type uniformFixedValue;", "no 'uniformValue'"),
    ("type flowRateInletVelocity; massFlowRate 1; rho rho;", "massFlowRate"),
    ("type flowRateInletVelocity; volumetricFlowRate 1; extrapolateProfile yes;", "extrapolateProfile"),
    ("type flowRateInletVelocity;", "no 'volumetricFlowRate'"),
    ("type fixedValue; value nonuniform List<vector> 2 ((0 0 1) (0 0 1));", "holds 2 vectors"),
    ("type inletOutlet; inletValue uniform (0 0 0);", "inletOutlet"),
])
def test_each_refusal_is_raised_by_name(prod, tmp_path, text, word):
    dst = write_case(tmp_path, block_mesh(), "        " + text.replace("; ", ";\n        "))
    with pytest.raises(prod.FoamYadeError, match=re.escape(word)):
        prod.FoamCase(dst, prod.FY_SOLVER_ICO)


def test_a_malformed_function_is_refused_when_the_solver_is_made(prod, tmp_path):
    """the reader hands the table on as written; the library's own check names what is wrong with it (tests/test_inlets.py: refusals)"""
    dst = write_case(tmp_path, block_mesh(), "        type uniformFixedValue;\n        uniformValue table ((0 (0 0 1)) (0 (0 0 2)));")
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    assert np.isnan(prod.time_function_eval(fc.case.inlets.inlets[0].terms[0].f, 0.0))
    fc.close()


def test_a_restarted_case_evaluates_the_function_at_the_restart_time(prod, tmp_path):
    """a time directory written from host arrays keeps the entry with its function dictionary; opened from it, the case's start_time is that directory's and the inlet's
    value there is the function's value at that time"""
    mesh = block_mesh()
    dst = write_case(tmp_path, mesh, "        type uniformFixedValue;\n        " + SINE)
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    n = NX * NY * NZ
    fc.write_fields("0.035", np.zeros((n, 3)), np.zeros(n))
    fc.close()
    text = (dst / "0.035/U").read_text()
    assert "uniformFixedValue" in text and "uniformValue" in text and "sine" in text and "frequency 4" in text
    (dst / "system/controlDict").write_text((dst / "system/controlDict").read_text().replace("startFrom       startTime;", "startFrom       latestTime;"))
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    d = fc.case.inlets
    assert fc.start_name == "0.035" and d.start_time == 0.035 and d.n == 1
    Sf = np.tile([0.0, 0.0, -0.01], (NX * NY, 1))
    got, want = eval_inlet(prod, d, NX * NY, Sf, d.start_time), ir.inlet_values(SINE_TERMS, 0.035, Sf)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max() and np.abs(want - ir.inlet_values(SINE_TERMS, 0.0, Sf)).max() > 0.01
    fc.close()


# ------------------------------------------------------------------------------------------------ GPU: through foamYadeHip, and restarted
def run_exe(prod, dst):
    exe = os.path.join(os.path.dirname(prod.__file__), "bin", "foamYadeHip")
    if not os.path.exists(exe):
        pytest.fail("foamYadeHip has not been built: run __graft_entry__.build()")
    out = subprocess.run([exe, "-solver", "ico", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def written_value(path, patch):
    """the `value nonuniform List<vector>` of `patch` in a written ASCII field file"""
    t = open(path).read()
    t = t[t.index("boundaryField"):]
    t = t[t.index(patch):]
    m = re.search(r"value\s+nonuniform List<vector> (\d+)\s*\(", t)
    body = t[m.end():]
    rows = re.findall(r"\(([^()]+)\)", body[:body.index("\n)")])
    v = np.array([[float(x) for x in r.split()] for r in rows[:int(m.group(1))]])
    assert len(v) == int(m.group(1))
    return v


@pytest.mark.gpu
def test_spouted_bed_block_case_runs_and_restarts(prod, tmp_path):
    """a jet through part of the bottom side of a block (nonuniform fixedValue, constant/polyMesh with scrambled numbering) through foamYadeHip for three steps: the
    written entry is the jet, face for face, and a solver started from the written directory carries the bits of an uninterrupted run -- fields and boundary values"""
    mesh = block_mesh()
    place = zmin_lattice_place(mesh)
    jet = np.zeros((NX * NY, 3)); jet[:, 2] = 0.05
    jet[(place % NX < 2) & (place // NX < 2), 2] = 0.6                  # the spout: a 2 x 2 corner of the bottom
    jet += np.random.RandomState(3).uniform(-0.01, 0.01, jet.shape)
    dst = write_case(tmp_path, mesh, "        type fixedValue;\n        value " + vec_list(jet) + ";")
    assert "End" in run_exe(prod, dst)
    assert sorted(d for d in os.listdir(dst) if d[0].isdigit()) == ["0", "0.015"]
    text = (dst / "0.015/U").read_text()
    assert re.search(r"zmin\s*\{\s*type fixedValue;", text)
    assert np.array_equal(written_value(dst / "0.015/U", "zmin"), jet)
    # the uninterrupted run, driven from Python
    fc = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    s = prod.Solver(fc.case)
    U0, p0 = fc.initial_fields()
    s.set("U", U0); s.set("p", p0)
    for _ in range(3):
        s.step()
    (dst / "system/controlDict").write_text((dst / "system/controlDict").read_text().replace("startFrom       startTime;", "startFrom       latestTime;"))
    fr = prod.FoamCase(dst, prod.FY_SOLVER_ICO)
    assert fr.start_name == "0.015" and fr.case.inlets.start_time == 0.015
    U, p = fr.initial_fields()
    np.testing.assert_array_equal(U, s.get("U").reshape(-1, 3)); np.testing.assert_array_equal(p, s.get("p"))
    r = prod.Solver(fr.case)
    r.set("U", U); r.set("p", p)
    assert np.array_equal(r.get("U_boundary"), s.get("U_boundary"))
    z0 = 2 * (NY * NZ + NX * NZ)
    want = np.zeros_like(jet); want[place] = jet
    assert np.array_equal(r.get("U_boundary").reshape(-1, 3)[z0:z0 + NX * NY], want) and np.abs(U).max() > 0.1
    r.step(); s.step()                  # (the inlet's faces: phi is not among the written fields, so the two runs' interiors part in the last digits from here on)
    assert np.array_equal(r.get("U_boundary").reshape(-1, 3)[z0:z0 + NX * NY], s.get("U_boundary").reshape(-1, 3)[z0:z0 + NX * NY])
    for o in (s, r, fc, fr):
        o.close()


@pytest.mark.gpu
def test_general_mesh_case_with_a_function_runs_and_restarts(prod, tmp_path):
    """uniformFixedValue with a sine on a prism mesh through foamYadeHip for three steps: the written entry keeps its type and function dictionary, its value is the
    faces' current value (the function at 0.015), and the restarted case continues the function at its own time"""
    mesh = pm.prism_block(3, 3, 4, LEN, vertex_map=pm.wavy(0.01, LEN))
    n = int(mesh["patch_size"][ZMIN])
    dst = write_case(tmp_path, mesh, "        type uniformFixedValue;\n        " + SINE)
    assert "general polyhedral mesh" in run_exe(prod, dst)
    text = (dst / "0.015/U").read_text()
    assert "uniformFixedValue" in text and "sine" in text and "frequency 4" in text
    Sf = np.zeros((n, 3))
    at = lambda t: ir.inlet_values(SINE_TERMS, t, Sf)
    got = written_value(dst / "0.015/U", "zmin")
    assert got.shape == (n, 3) and np.abs(got - at(0.015)).max() <= 1e-14 * np.abs(at(0.015)).max()
    (dst / "system/controlDict").write_text((dst / "system/controlDict").read_text().replace("startFrom       startTime;", "startFrom       latestTime;"))
    fr = prod.GeneralFoamCase(dst)
    assert fr.start_name == "0.015" and fr.ldu_case.inlets.start_time == 0.015
    r = prod.LduSolver.from_foam_case(fr)
    ni, s0 = len(mesh["neighbour"]), int(mesh["patch_start"][ZMIN])
    inlet = lambda: r.get("U_boundary")[s0 - ni:s0 - ni + n]
    # the restart's boundary values are the function at the directory's time, 0.015 as read; the run wrote it at 0.005 + 0.005 + 0.005 as summed: one rounding apart
    assert np.abs(inlet() - got).max() <= 1e-14 * np.abs(got).max()
    r.step()
    assert np.abs(inlet() - at(0.02)).max() <= 1e-14 * np.abs(at(0.02)).max() and np.abs(at(0.02) - at(0.015)).max() > 0.01
    r.close(); fr.close()
