"""The inlets' reference and host arithmetic, without a GPU: fy_time_function_eval against the numpy restatement in tests/inlets_ref.py, the descriptors' layout,
and the split-patch, rebuild-per-step reference against a plain oracle run (bit for bit with a constant uniform value): the restatement the device is held to must
itself be right."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import inlets_ref as ir
import poly_meshes as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = dict(kind="table", points=[(0.5, 1.0), (1.0, -2.0), (1.75, 0.25), (4.0, 3.0)])
TABLE_REPEAT = dict(TABLE, out_of_bounds="repeat")
SINE = dict(kind="sine", amplitude=0.7, frequency=3.0, t0=0.125)
SQUARE = dict(kind="square", amplitude=2.0, frequency=0.5, t0=0.25)
SQUARE_MS = dict(kind="square", amplitude=-1.5, frequency=4.0, t0=0.0, mark_space=3.0)


def both(product, spec, t):
    return product.time_function_eval(spec, t), ir.time_function(spec, t)


def agree(product, spec, times):
    for t in times:
        lib_v, ref_v = both(product, spec, t)
        assert abs(lib_v - ref_v) <= 1e-14 * max(abs(ref_v), 1e-300) or lib_v == ref_v, (spec, t, lib_v, ref_v)


def test_constant_and_sine(product):
    agree(product, 1.25, [-1.0, 0.0, 7.5])
    agree(product, dict(kind="constant", value=-3.5), [0.0, 2.0])
    agree(product, SINE, np.linspace(-1.0, 3.0, 41))
    assert product.time_function_eval(SINE, 0.125) == 0.0
    assert product.time_function_eval(SINE, 0.125 + 1.0 / 12.0) == pytest.approx(0.7, rel=1e-14)      # a quarter period on


def test_table_interior_knots_ends_clamp_and_repeat(product):
    knots = [p[0] for p in TABLE["points"]]
    interior = [0.6, 0.999, 1.3, 1.7500001, 2.875, 3.999]
    agree(product, TABLE, knots + interior + [-5.0, 0.49999, 4.00001, 100.0])
    agree(product, TABLE_REPEAT, knots + interior + [-5.0, -0.2, 0.49999, 4.00001, 4.6, 7.5, 8.3, 100.0])
    for t, v in TABLE["points"]:                                       # the knots carry their own values exactly
        assert product.time_function_eval(TABLE, t) == v
    assert product.time_function_eval(TABLE, -5.0) == 1.0 and product.time_function_eval(TABLE, 100.0) == 3.0      # clamp
    assert product.time_function_eval(TABLE, 2.875) == 0.25 + (3.0 - 0.25) * 0.5
    # repeat: the table's span is 3.5; a time one or two spans off the range lands on the same value
    for t in (0.6, 1.3, 2.875):
        assert product.time_function_eval(TABLE_REPEAT, t + 3.5) == pytest.approx(product.time_function_eval(TABLE, t), rel=1e-13)
        assert product.time_function_eval(TABLE_REPEAT, t - 7.0) == pytest.approx(product.time_function_eval(TABLE, t), rel=1e-13)
    assert product.time_function_eval(dict(kind="table", points=[(1.0, 4.0)]), 9.0) == 4.0


def test_square_wave_switching_instants_and_mark_space(product):
    # frequency 0.5, t0 0.25: +2 on [0.25, 1.25), -2 on [1.25, 2.25), the switch belongs to the half that starts there
    for t, v in ((0.25, 2.0), (1.0, 2.0), (1.25, -2.0), (2.0, -2.0), (2.25, 2.0), (-0.75, -2.0), (-1.75, 2.0)):
        assert product.time_function_eval(SQUARE, t) == v, t
    agree(product, SQUARE, np.linspace(-3.0, 5.0, 65))
    # markSpace 3: three quarters of each period of 0.25 up (amplitude -1.5: "up" is -1.5)
    for t, v in ((0.0, -1.5), (0.18, -1.5), (0.1875, 1.5), (0.24, 1.5), (0.25, -1.5), (0.4375, 1.5)):
        assert product.time_function_eval(SQUARE_MS, t) == v, t
    agree(product, SQUARE_MS, np.linspace(-1.0, 1.0, 129))


def test_malformed_functions_evaluate_to_nan(product):
    bad = [dict(kind="table", points=[(0.0, 1.0), (0.0, 2.0)]), dict(kind="table", points=[(1.0, 1.0), (0.5, 2.0)]), dict(kind="sine", frequency=0.0),
           dict(kind="square", frequency=-1.0), dict(kind="table", points=[(0.0, 1.0)], out_of_bounds="repeat"), dict(kind="table", points=[(0.0, 1.0)], out_of_bounds=3),
           dict(kind=9)]
    for spec in bad:
        assert math.isnan(product.time_function_eval(spec, 0.3)), spec


def test_descriptor_layout_and_symbols(product):
    """the ctypes mirror states the header's layout (the static_asserts of csrc/inlets.hpp state the same sizes), and the library exports the entry points"""
    assert C.sizeof(product.TimeFunction) == 72 and C.sizeof(product.InletTerm) == 88 and C.sizeof(product.InletDesc) == 272 and C.sizeof(product.InletsDesc) == 24
    assert product.CaseDesc.inlets.size == 24 and product.LduCase.inlets.size == 24
    L = product.lib()
    for name in ("fy_solver_set_inlets", "fy_ldu_solver_set_inlets", "fy_time_function_eval"):
        assert hasattr(L, name)
    hdr = open(os.path.join(ROOT, "include", "foamyade_hip.h")).read()
    assert L.fy_abi_version() == int(re.search(r"#define FY_ABI_VERSION (\d+)", hdr).group(1)) >= 27
    d = product.inlets_desc([dict(patch=4, terms=[dict(f=TABLE, shape=(0, 0, 1.0)), dict(f=2.0, shape="flow_rate"), dict(f=SINE, shape=np.ones((5, 3)))])], start_time=1.5)
    assert d.n == 1 and d.start_time == 1.5 and d.inlets[0].patch == 4 and d.inlets[0].n_terms == 3
    t = d.inlets[0].terms
    assert [t[m].shape_kind for m in range(3)] == [product.SHAPE_UNIFORM, product.SHAPE_FLOW_RATE, product.SHAPE_PER_FACE]
    assert t[0].f.kind == product.TIME_TABLE and t[0].f.n_points == 4 and t[0].f.points[3] == -2.0 and t[1].f.value == 2.0 and t[2].f.frequency == 3.0


def test_inlet_values_and_flow_rate_shape():
    Sf = np.array([[0, 0, -0.5], [0, 0, -0.25], [0.0, 0.3, -0.4]])
    S = ir.flow_rate_shape(Sf)
    np.testing.assert_allclose(np.einsum("fa,fa->", S, Sf), -1.0, rtol=1e-15)          # a unit coefficient carries a unit flow INTO the domain
    v = ir.inlet_values([dict(f=SINE, shape=(0, 0, 2.0)), dict(f=3.0, shape="flow_rate")], 0.4, Sf)
    np.testing.assert_allclose(v, ir.time_function(SINE, 0.4) * np.array([0, 0, 2.0]) + 3.0 * S, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ the split-patch, rebuild-per-step reference
def _mesh(kind):
    if kind == "hexahedra":
        return pm.hex_block(4, 3, 5, (1.0, 0.8, 1.2))
    if kind == "wavy_renumbered":
        return pm.hex_block(4, 3, 5, (1.0, 0.8, 1.2), pm.wavy(0.03, (1.0, 0.8, 1.2)), renumber_seed=5)
    return pm.prism_block(3, 3, 4, (1.0, 0.9, 1.1), vertex_map=pm.wavy(0.02, (1.0, 0.9, 1.1)))


U_BC, P_BC = [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1]          # inflow on zmin (patch 4), fixed pressure on zmax, walls elsewhere
V_IN = (0.02, -0.01, 0.3)


def _u_val(v=V_IN):
    return [(0, 0, 0)] * 4 + [tuple(v), (0, 0, 0)]


@pytest.mark.parametrize("kind", ["hexahedra", "wavy_renumbered", "prisms"])
@pytest.mark.parametrize("solver", [0, 1])
def test_split_patch_rebuild_reproduces_a_plain_run_bit_for_bit(oracle, kind, solver):
    """a constant uniform value through the split patch and the per-step rebuild = the plain oracle run, both solvers: U, p, phi to the bit after four steps"""
    mesh = _mesh(kind)
    kw = dict(n_non_orth=1, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, solver=solver)
    if solver == 1:
        kw.update(n_outer=2, g=(0.0, 0.0, -0.5))
    U0 = np.random.RandomState(3).rand(mesh["n_cells"], 3) * 0.05
    plain = oracle.LduSolver(mesh, 0.02, 0.01, U_BC, _u_val(), P_BC, **kw)
    plain.set("U", U0)
    n = int(mesh["patch_size"][4])
    run = ir.SplitPatchRun(oracle, mesh, 4, 0.02, 0.01, U_BC, _u_val((9.0, 9.0, 9.0)), P_BC, None, lambda t: np.tile(V_IN, (n, 1)), U0=U0, **kw)
    assert np.array_equal(run.get("phi"), plain.get("phi"))
    for s in range(4):
        plain.step()
        run.step(0.02 * (s + 1))
    for f in ("U", "p", "phi"):
        assert np.array_equal(run.get(f), plain.get(f)), f
    assert np.abs(plain.get("U")).max() > 0.1
    plain.close()


def test_split_patch_rebuild_with_kEqn_bit_for_bit(oracle):
    mesh = _mesh("wavy_renumbered")
    kw = dict(n_non_orth=1, p_tol=1e-10, p_rel_tol=0.0, p_final_tol=1e-10, u_tol=1e-10, solver=1, turbulence_model=2, k_initial=1e-3, nut_initial=1e-4, k_tol=1e-10,
              nut_bc=[0] * 6, nut_val=[0.0] * 6, k_bc=[0, 0, 0, 0, 1, 0], k_val=[0, 0, 0, 0, 2e-3, 0])
    U0 = np.random.RandomState(4).rand(mesh["n_cells"], 3) * 0.05
    plain = oracle.LduSolver(mesh, 0.02, 0.01, U_BC, _u_val(), P_BC, **kw)
    plain.set("U", U0)
    n = int(mesh["patch_size"][4])
    run = ir.SplitPatchRun(oracle, mesh, 4, 0.02, 0.01, U_BC, _u_val(), P_BC, None, lambda t: np.tile(V_IN, (n, 1)), U0=U0, **kw)
    for s in range(4):
        plain.step()
        run.step(0.02 * (s + 1))
    for f in ("U", "p", "phi", "nut", "k"):
        assert np.array_equal(run.get(f), plain.get(f)), f
    assert np.abs(plain.get("k") - 1e-3).max() > 1e-6
    plain.close()
