"""The case list that tests/test_mg_reference.py (CPU oracle) and tests/test_mg_parity.py (HIP solver) hold to tests/mg_ref.py: one step of a lid cavity
from a random velocity field, so that rAU -- and with it every pressure coefficient -- varies from cell to cell.  Each size is there for the branch
of the block pressure solver it reaches."""
import numpy as np

import mg_ref

CUTS = (1, 2, 3, 6)                       # solve_p is cut at these iteration counts (p_tol = p_final_tol = 1e-30, p_rel_tol = 0: the count alone ends a solve)


def _sizes(n, ratio, length):             # the wall-refined block of test_graded_cavity_steps_match_oracle
    half_n = n // 2
    r = ratio ** (1.0 / (half_n - 1))
    h = r ** np.arange(half_n)
    half = h * (0.5 * length / h.sum())
    return np.concatenate([half, half[::-1]])


def _lid():
    u_val = [(0, 0, 0)] * 6
    u_val[3] = (1.0, 0, 0)
    return dict(u_bc=[0] * 6, u_val=u_val)


#  id                 dims            what it reaches
CASES = {
    "4x4x4": dict(dims=(4, 4, 4)),                                        # one level: M^-1 = A^-1
    "8x8x8": dict(dims=(8, 8, 8)),                                        # two levels, all inside the one-workgroup tail
    "13x9x7": dict(dims=(13, 9, 7), p_ref_cell=408),                      # odd edges throughout, reference cell (5, 4, 3)
    "16x16x4": dict(dims=(16, 16, 4)),                                    # coarsest 8 x 8 x 2 = 128 cells, band 64: both direct-solve limits at equality
    "16x16x5": dict(dims=(16, 16, 5)),                                    # 1280 cells: level 0 outside the tail
    "20x20x20": dict(dims=(20, 20, 20)),                                  # tail of 10^3 + 5^3
    "40x12x6": dict(dims=(40, 12, 6)),                                    # an edge over 8 forces a fourth level
    "33x17x9": dict(dims=(33, 17, 9)),                                    # larger odd block
    "4x4x512": dict(dims=(4, 4, 512)),                                    # level 1 = 2 x 2 x 256 = 1024 cells with 6 levels left: both tail limits at equality
    "14x10x6_fixed_p": dict(dims=(14, 10, 6), u_bc=[1, 0, 0, 0, 0, 0], p_bc=[1, 0, 0, 0, 0, 0], p_val=[0.3, 0, 0, 0, 0, 0]),      # no reference cell
    "12x12x12_pimple": dict(dims=(12, 12, 12), solver=1, g=(0, 0, -9.81), p_bc=[2] * 6, dx=0.1 / 12, dt=1e-3, nu=1e-6, lid=False),
    "14x14x14_graded": dict(dims=(14, 14, 14), dt=0.01, grading=(_sizes(14, 4.0, 1.0), _sizes(14, 4.0, 1.0), _sizes(14, 2.5, 0.8))),
}


def case_kwargs(name, p_solver=1, p_max_iter=6):
    """(positional arguments, keyword arguments) that oracle.fv_case and product.make_case share"""
    c = CASES[name]
    nx, ny, nz = c["dims"]
    kw = dict(_lid()) if c.get("lid", True) else {}
    for k in ("u_bc", "p_bc", "p_val", "g", "grading", "p_ref_cell"):
        if k in c:
            kw[k] = c[k]
    kw.update(p_solver=p_solver, p_max_iter=p_max_iter, p_tol=1e-30, p_final_tol=1e-30, p_rel_tol=0.0)
    return (c.get("solver", 0), nx, ny, nz, c.get("dx", 0.05), c.get("dt", 0.004), c.get("nu", 0.01)), kw


def ref_cell(name):
    """the pressure reference cell, or None where a fixed-value pressure side stands in for it"""
    c = CASES[name]
    return None if 1 in c.get("p_bc", []) else c.get("p_ref_cell", 0)


def initial_U(name):
    nx, ny, nz = CASES[name]["dims"]
    return np.random.RandomState(3).rand(nx * ny * nz, 3) * 0.2


def stepped(make_case, make_solver, name, **kw):
    """a solver of `name` after the one step that assembles its pressure matrix"""
    args, ckw = case_kwargs(name, **kw)
    s = make_solver(make_case(*args, **ckw))
    s.set("U", initial_U(name))
    s.step()
    return s


def vectors(n, diag_scale):
    """the right-hand sides the preconditioner is applied to (random, smooth), and a PCG problem with a start vector whose mean is not zero"""
    rs = np.random.RandomState(11)
    t = (np.arange(n) + 0.5) / n
    return dict(random=rs.randn(n), smooth=np.cos(3.0 * np.pi * t) + 0.3 * np.sin(11.0 * np.pi * t * t) + 0.25,
                b=rs.randn(n) * diag_scale, x0=0.1 * rs.rand(n) + 0.05)


def hierarchy(solver, name, dims=None):
    """the reference hierarchy from a solver's own level-0 coefficients"""
    d = dims or CASES[name]["dims"]
    return mg_ref.Hierarchy(solver.get("p_diag"), solver.get("p_ux"), solver.get("p_uy"), solver.get("p_uz"), d, ref_cell(name))


def rel(a, ref):
    """max |a - ref| / max |ref|"""
    ref = np.asarray(ref, np.longdouble)
    return float(np.abs(np.asarray(a, np.longdouble) - ref).max() / np.abs(ref).max())


def residual_scale(H, x_scale, b, x0):
    """how far the reported residual sum|r| / normFactor moves when the iterate moves by x_scale in every cell: sum over the rows of |A| x_scale / normFactor"""
    L = H.levels[0]
    rows = np.abs(L.diag).copy()
    for a, ax in ((L.ux, 2), (L.uy, 1), (L.uz, 0)):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[ax] = slice(0, -1); hi[ax] = slice(1, None)
        rows[tuple(lo)] += np.abs(a[tuple(lo)]); rows[tuple(hi)] += np.abs(a[tuple(lo)])
    x0 = np.asarray(x0, np.longdouble); b = np.asarray(b, np.longdouble)
    pA = H.apply(np.full(x0.shape, x0.mean(), np.longdouble))
    norm = (np.abs(H.apply(x0) - pA) + np.abs(b - pA)).sum() + 1e-20
    return float(rows.sum() * x_scale / norm)
