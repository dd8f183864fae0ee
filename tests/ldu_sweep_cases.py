"""The case list and the protocol that tests/test_ldu_sweeps_reference.py (both builds of the CPU oracle) and tests/test_ldu_sweeps_parity.py (the HIP solver)
share: the FV sweeps of the general-mesh solver -- csrc/ldu_kernels.hip and the driver in ldu_solver.cpp -- held to oracle/ldu_oracle.cpp compiled in long
double.  The block solver's list is tests/fv_sweep_cases.py; the bound (FACTOR, E_WINDOW) and the envelope are the project's and are taken from there.

Protocol of a case.  Every iteration count is frozen (u_tol = u_rel_tol = 0 with u_max_iter = k_u; p_tol = p_rel_tol = p_final_tol = p_final_rel_tol = 0 with
p_max_iter = k_p; likewise k / epsilon: both sides' solve_vec3 / solve_momentum and solve_pressure then stop on the count), so a step is a fixed chain of
operations and both sides can be held to rounding.  The pressure solver is the Jacobi-preconditioned PCG (the oracle has no multigrid; the V-cycle is pinned by
tests/test_amg_parity.py).  U (0 .. 0.05) and p start from seeded random fields, two steps run.  A coupled (pimpleFoamYade) case hands alpha / uSourceDrag /
uSource to the oracle through step(source, alpha, drag): on the GPU they are the device's own (a few hundred clustered particles, hold_sources keeps them
readable after the step), so the FV halves of both sides see the same bits; without a GPU they are seeded random fields.  The distance of a field is
max |x - wide| / max |wide|.

Each case is there for the branch of a kernel or of the driver that it reaches; `omit` lists the names a case leaves out, with the reason; `zero` the names
that are identically zero on it.

Not in this list, because oracle/ldu_oracle.cpp does not carry them: the T equation (tests/test_ldu_heat.py), meanVelocityForce (tests/test_flow_control.py)
and the wall loads (tests/test_wall_loads.py).  They keep their own tests.  (Wall functions are carried -- nearWallDist, the wall cells' production and imposed
epsilon: pimple_through_flow_kEpsilon_wall_functions; the case reader's rules for them stay in tests/test_ldu_wall_functions.py.)"""
import numpy as np

import golden_cases as gc
import poly_meshes as pm
import fv_sweep_cases as fc
from fv_sweep_cases import E_WINDOW, FACTOR, rel, worst  # noqa: F401  (the project's bound, one statement of it)

FV, ZG, SLIP = 0, 1, 2            # velocity patch types
PZG, PFV, PFLUX = 0, 1, 2         # pressure patch types
H = 0.01                          # edge of a (coarse) lattice cell: every box is dims * H

# ---- what is compared (the device's names), by the point of the step at which it is final -----------------------------------------------------------
GROUPS = {
    "geometry": ("C", "V", "Cf", "Sf", "magSf", "w", "dcNO", "kvec", "sep"),
    "assembled": ("mom_diag", "mom_b", "gradP", "divT", "ddtU", "rAU", "rAUf"),                      # before any solve of the momentum assembly that wrote them
    "neighbours": ("mom_lower", "mom_upper"),                                                        # own group: a limited scheme's weight divides two differences of magSqr(U)
    "predicted": ("HbyA", "phiForces", "p_diag", "p_coef", "p_rhs"),                                 # after the predictor
    "fluxHbyA": ("phiHbyA",),                                                                        # ddtCorr's coefficient divides by |phi|
    "solved": ("U", "p", "phi", "vGrad", "nut", "k", "epsilon"),                                     # after the pressure solve (and the closure's correct())
}
GROUP_OF = {nm: grp for grp, names in GROUPS.items() for nm in names}
GEOMETRY = GROUPS["geometry"]
NEVER_OMITTED = ("U", "p", "phi", "rAU", "p_diag", "p_coef")
# The device keeps the momentum matrix in the form its sweeps read: mom_diag with the patches' internal coefficients added (fvMatrix::addBoundaryDiag of the
# scalar part: k_ldu_mom_cells / k_ldu_pmom_cells, `dg += gm`, `dg += phi`) and mom_b with the patches' boundary coefficients added (addBoundarySource).  The
# oracle keeps the four apart (diag, bint, src, bsrc) as fvMatrix does and forms the sums where it uses them (Ldu::dgc, Ldu::total_source): the copy-out names
# mom_dg and mom_b are those two functions.  grad(U): the device has one array, which the second outer corrector and the closure's correct() overwrite; the
# oracle keeps the assembly's (vGradNow) apart from the coupling's (vGrad), which correct() overwrites
ORACLE_NAME = {"mom_diag": "mom_dg"}


def oracle_name(c, nm):
    if nm == "vGrad":
        return "vGrad" if c["kw"].get("turbulence_model") else "vGradNow"
    return ORACLE_NAME.get(nm, nm)


R_STORAGE = "kEqn / kEpsilon assemble and solve their transport equations in the momentum matrix's storage (and iterate in HbyA's) after the last corrector"
R_ICO = "icoFoamYade forms none of the coupling's input fields nor phicForces: the device holds no such array"
R_NO_CLOSURE = "no turbulence model"
R_NO_EPS = "no epsilon equation"
R_NO_K = "no k equation"
R_NO_CYCLIC = "no cyclic patches: neither side holds image offsets"
R_KVEC_NOISE = ("an orthogonal mesh: nonOrthCorrectionVectors = n - d / (n & d) is what rounding leaves of 0, a few ulp of 1 (up to 3e-15) or exactly zero "
                "by the face; a distance relative to its maximum does not exist (that it stays below 100 ulp = 2.2e-14 on every side is asserted instead)")
KVEC_NOISE = 100 * 2.0 ** -52


def _turn(a=0.5, b=-0.35, c=0.8):
    """the rotation of tests/test_ldu_parity.py: every face of a symmetry patch with its own oblique normal"""
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


R = _turn()
IN_OUT = [("inlet", [0]), ("outlet", [1]), ("walls", [2, 3]), ("sides", [4, 5])]


def box(dims):
    return tuple(n * H for n in dims)


def then(*maps):
    def m(P):
        for f in maps:
            if f is not None:
                P = f(P)
        return P
    return m


turned = lambda P: P @ R.T  # noqa: E731

# ---- meshes: name -> (dims, builder(dims, L, vertex_map), vertex_map(L)); the vertex map also carries the particles into the mesh ---------------------
WAVY_DIMS = (9, 7, 5)             # 315 cells, 802 internal and 286 boundary faces: more than one 256-thread block with a ragged last one on all three
MESHES = {
    "lattice": ((6, 5, 4), lambda d, L, vm: pm.hex_block(*d, L), lambda L: None),
    "sheared": ((6, 5, 4), lambda d, L, vm: pm.hex_block(*d, L, vm, renumber_seed=21), lambda L: pm.shear(0.3, 0.1, 0.2)),
    "wavy": (WAVY_DIMS, lambda d, L, vm: pm.hex_block(*d, L, vm, renumber_seed=3), lambda L: pm.wavy(0.2 * H, L)),
    "wavy_in_out": (WAVY_DIMS, lambda d, L, vm: pm.hex_block(*d, L, vm, patches=IN_OUT, renumber_seed=1), lambda L: pm.wavy(0.2 * H, L)),
    "wavy_turned": (WAVY_DIMS, lambda d, L, vm: pm.hex_block(*d, L, vm, renumber_seed=12), lambda L: then(pm.wavy(0.2 * H, L), turned)),
    "prisms": ((6, 5, 4), lambda d, L, vm: pm.prism_block(*d, L, vm), lambda L: pm.wavy(0.15 * H, L)),
    "tetrahedra": ((5, 4, 3), lambda d, L, vm: pm.tet_block(*d, L, vm), lambda L: pm.wavy(0.1 * H, L)),
    "refined": ((8, 8, 6), lambda d, L, vm: pm.refined_block(*d, 3, L, vm), lambda L: pm.wavy(0.05 * H, L)),
    # the box of amg_cases._cyclic (10 x 8 x 6, periodically distorted, x and z sides paired) at this list's cell size
    "cyclic": ((10, 8, 6), lambda d, L, vm: pm.make_cyclic(pm.hex_block(*d, L, vm), [(0, 1), (4, 5)]), lambda L: pm.wavy_periodic(0.2 * H, L)),
    "chain": ((3, 1, 1), lambda d, L, vm: pm.hex_block(*d, L), lambda L: None),
}
ORTHOGONAL = ("lattice", "chain")
_built = {}


def mesh_of(c):
    k = c["mesh"]
    if k not in _built:
        dims, build, vmap = MESHES[k]
        _built[k] = build(dims, box(dims), vmap(box(dims)))
    return _built[k]


def counts_of(mesh):
    """(cells, faces, internal faces) as the solvers number them: a cyclic pair is one internal face"""
    nf, ni = len(mesh["owner"]), len(mesh["neighbour"])
    pn = mesh.get("patch_neighbour")
    if pn is not None:
        folded = sum(int(mesh["patch_size"][a]) for a, b in enumerate(pn) if b > a)
        nf, ni = nf - 2 * folded + folded, ni + folded
    return int(mesh["n_cells"]), nf, ni


# ---- boundary sets (six patches in poly_meshes.SIDES order unless said) --------------------------------------------------------------------------
def cavity(lid=(1.0, 0.0, 0.0)):
    u_val = [(0.0, 0.0, 0.0)] * 6
    u_val[3] = tuple(lid)
    return dict(u_bc=[FV] * 6, u_val=u_val, p_bc=[PZG] * 6)


def closed_box(g=(0.0, 0.0, -9.81)):
    """no-slip walls, fixedFluxPressure, gravity"""
    return dict(g=tuple(g), u_bc=[FV] * 6, u_val=[(0.0, 0.0, 0.0)] * 6, p_bc=[PFLUX] * 6)


def through_flow(u_in, fixed_outlet=True):
    """IN_OUT patches: inlet fixedValue, outlet zeroGradient, no-slip walls, zeroGradient sides; the outlet's pressure fixed (no reference cell) or not (adjustPhi)"""
    return dict(u_bc=[FV, ZG, FV, ZG], u_val=[(u_in, 0.0, 0.0)] + [(0.0, 0.0, 0.0)] * 3, p_bc=[PZG, PFV if fixed_outlet else PZG, PZG, PZG], p_val=[0.0] * 4)


def symmetry_sides(pimple):
    lid = tuple(R @ (np.array([0.05, 0, 0.02]) if pimple else np.array([1.0, 0, 0.3])))
    u_val = [(0.0, 0.0, 0.0)] * 6
    u_val[3] = lid
    out = dict(u_bc=[SLIP, SLIP, SLIP, FV, FV, FV], u_val=u_val, p_bc=[PZG, PZG, PZG] + ([PFLUX] * 3 if pimple else [PZG] * 3))
    if pimple:
        out["g"] = tuple(R @ np.array([0.0, 0.0, -9.81]))
    return out


def periodic(pimple):
    """x and z sides cyclic (their entries are unused), the y sides walls: a moving one in icoFoamYade, gravity towards one in pimpleFoamYade"""
    u_val = [(0.0, 0.0, 0.0)] * 6
    if not pimple:
        u_val[3] = (1.0, 0.0, 0.4)
        return dict(u_bc=[ZG, ZG, FV, FV, ZG, ZG], u_val=u_val, p_bc=[PZG] * 6)
    return dict(g=(0.0, -9.81, 0.0), u_bc=[ZG, ZG, FV, FV, ZG, ZG], u_val=u_val, p_bc=[PZG, PZG, PFLUX, PFLUX, PZG, PZG])


CASES = {}


def add(name, solver, mesh, bcs, k_u=3, k_p=4, u0="random", source=False, particles=(300, 80), radius_dx=0.3, omit=None, zero=(), **kw):
    """kw: controls in the oracle's spelling (oracle.LduSolver), shared by both sides.  particles: (spread over the box, packed into a 2 H cube)"""
    assert name not in CASES and mesh in MESHES
    kw = dict(bcs, **kw)
    kw.setdefault("n_correctors", 2)
    kw.setdefault("n_non_orth", 0 if mesh in ORTHOGONAL else 1)
    # time step and viscosity put the three parts of the momentum matrix within an order of magnitude of each other, as fv_sweep_cases.add does on cells of the
    # same size: U up to 0.05, or the lid's 1, on cells of 0.01 (Courant number and diffusion number 0.02 .. 0.2 beside the time derivative's 1), so that a
    # defect in any of them shows; the closures keep a viscosity their nut can matter beside
    kw.setdefault("dt", 5e-3 if solver == 1 else 1e-3)
    kw.setdefault("nu", (1e-5 if kw.get("turbulence_model") else 2e-4) if solver == 1 else 0.01)
    zero = tuple(zero)
    omit = dict(omit or {})
    if mesh in ORTHOGONAL:
        omit["kvec"] = R_KVEC_NOISE
    CASES[name] = dict(name=name, solver=solver, mesh=mesh, k_u=k_u, k_p=k_p, u0=u0, source=source, particles=particles, radius_dx=radius_dx, kw=kw, omit=omit, zero=zero)


SCHEMES = ("linear", "upwind", "linearUpwind", "limitedLinear", "vanLeer", "MUSCL", "Minmod", "SuperBee", "QUICK")
BOTH = ((0, "ico", cavity()), (1, "pimple", closed_box()))
# ---- mesh kinds, each for the icoFoamYade cavity and the coupled pimpleFoamYade closed box
for kind in ("lattice", "sheared", "wavy", "prisms", "tetrahedra", "refined"):
    for solver, tag, bcs in BOTH:
        add(f"{tag}_{kind}", solver, kind, bcs, radius_dx=0.2 if kind == "tetrahedra" else 0.3)
for solver, tag in ((0, "ico"), (1, "pimple")):
    add(f"{tag}_cyclic", solver, "cyclic", periodic(solver))
    # two internal faces, every cell mostly boundary; three equations: PCG has solved them after its third iteration, so two are run
    add(f"{tag}_chain", solver, "chain", BOTH[solver][2], k_p=2, particles=(6, 0))
# ---- convection schemes 0 .. 8 on the wavy renumbered mesh; limitedLinear with k = 1 and 0.3
for q, nm in enumerate(SCHEMES):
    for solver, tag, bcs in BOTH:
        if q:                                                   # (linear: {tag}_wavy)
            add(f"{tag}_wavy_{nm}", solver, "wavy", bcs, convection_scheme=q)
        if q == 3:
            add(f"{tag}_wavy_{nm}_k03", solver, "wavy", bcs, convection_scheme=q, convection_limiter_k=0.3)
# the guard branches of the gradient ratio (NVDTVD::r): U uniform in half the box gives gradf = gradcf = 0 there and |gradcf| >= 1000 |gradf| beside it.  The uniform
# value is zero here, not ico_cavity_vanLeer_guard's (0.02, 0.01, 0.015): on a general mesh a uniform non-zero magSqr(U) has the Gauss gradient
# lPhi sum_f Sf / V, the rounding of a closed surface's zero, and its SIGN decides r = +-1999 -- the double and the wide build then take different limiters
# (distance 2e-1 in the neighbours group).  With zero the face values, the gradient and both differences are exactly zero on every mesh and in every width
add("ico_wavy_vanLeer_guard", 0, "wavy", cavity(), convection_scheme=4, u0="half_zero")
add("pimple_wavy_limitedLinear_guard", 1, "wavy", closed_box(), convection_scheme=3, u0="half_zero")
# ---- boundaries
add("ico_through_flow", 0, "wavy_in_out", through_flow(0.3))                                   # a fixed-value pressure patch: no reference cell
add("pimple_through_flow", 1, "wavy_in_out", dict(through_flow(0.03), g=(0.0, 0.0, -9.81)))
add("ico_free_outlet", 0, "wavy_in_out", through_flow(0.03, fixed_outlet=False))              # no patch fixes the pressure, the outlet leaves U free: adjustPhi scales the outflow
add("pimple_free_outlet", 1, "wavy_in_out", through_flow(0.03, fixed_outlet=False))
add("ico_symmetry_oblique", 0, "wavy_turned", symmetry_sides(0))
add("pimple_symmetry_oblique", 1, "wavy_turned", symmetry_sides(1), n_outer=2, u_relax=0.8, u_relax_final=1.0)      # (cmptMax / cmptMin of the vector coefficient in fvMatrix::relax)
add("ico_cyclic_vanLeer", 0, "cyclic", periodic(0), convection_scheme=4)                       # the limiter's d and the neighbour's IMAGE centre
add("pimple_cyclic_linearUpwind", 1, "cyclic", periodic(1), convection_scheme=2)
add("ico_wavy_source", 0, "wavy", cavity(), source=True)                                       # an external momentum source
add("ico_wavy_ref_cell", 0, "wavy", cavity(), p_ref_cell=200, p_ref_value=0.3)
add("pimple_wavy_ref_cell", 1, "wavy", closed_box(), p_ref_cell=314, p_ref_value=-0.2)
# ---- loop counts
for solver, tag, bcs in BOTH:
    for n_no in (0, 2):                                         # (1: every other case on a non-orthogonal mesh)
        add(f"{tag}_wavy_non_orth{n_no}", solver, "wavy", bcs, n_non_orth=n_no)
    for n_corr in (1, 3):
        add(f"{tag}_wavy_correctors{n_corr}", solver, "wavy", bcs, n_correctors=n_corr)
    add(f"{tag}_wavy_no_predictor", solver, "wavy", bcs, momentum_predictor=0)
add("pimple_wavy_outer2_relaxed", 1, "wavy", closed_box(), n_outer=2, u_relax=0.7, u_relax_final=1.0, p_relax=0.3, p_relax_final=1.0)
add("pimple_wavy_adjust_time_step", 1, "wavy", closed_box(), adjust_time_step=1, max_co=0.02, max_delta_t=0.1)
# ---- closures
KEQN = dict(turbulence_model=2, k_initial=1e-4, nut_initial=1e-5, k_tol=0.0, k_rel_tol=0.0, k_max_iter=3)
KEPS = dict(turbulence_model=3, k_initial=1e-4, eps_initial=1e-3, nut_initial=1e-5, k_tol=0.0, k_rel_tol=0.0, k_max_iter=3, eps_tol=0.0, eps_rel_tol=0.0, eps_max_iter=3)
CALCULATED = dict(k_bc=[0, 0, 0, 1, 0, 0], k_val=[0, 0, 0, 5e-4, 0, 0], nut_bc=[3, 0, 3, 3, 0, 1], nut_val=[1e-5, 0, 1e-5, 2e-5, 0, 5e-6])      # `calculated` nut patches, one fixed
add("pimple_wavy_smagorinsky", 1, "wavy", closed_box(), turbulence_model=1, nut_initial=1e-5, les_ck=0.2, nut_bc=[0, 0, 0, 1, 0, 0], nut_val=[0, 0, 0, 2e-5, 0, 0])
add("pimple_wavy_kEqn_linear", 1, "wavy", closed_box(), k_convection_scheme=0, **KEQN, **CALCULATED)
add("pimple_wavy_kEqn_upwind_relaxed", 1, "wavy", closed_box(), k_convection_scheme=1, k_relax=0.9, **KEQN, **CALCULATED)
add("pimple_wavy_kEpsilon", 1, "wavy", closed_box(), k_convection_scheme=1, eps_convection_scheme=1, eps_relax=0.8, eps_bc=[0, 0, 1, 1, 0, 0], eps_val=[0, 0, 2e-3, 3e-3, 0, 0], **KEPS, **CALCULATED)
# ---- closures on patches that carry a flux (fv_sweep_cases.py says what a closed box leaves out of the transport sweeps: the mode 0 / 1 / 2 path of
# ldu_kernels.hip and ldu_solver.cpp, the oracle's turb_eqn).  IN_OUT patches: inlet, outlet, walls, sides.  Every case names its k (and epsilon) scheme
TF = dict(through_flow(0.03), g=(0.0, 0.0, -9.81))
K_IN = dict(k_bc=[1, 0, 0, 0], k_val=[2e-4, 0, 0, 0])
E_IN = dict(eps_bc=[1, 0, 0, 0], eps_val=[2e-3, 0, 0, 0])
add("pimple_through_flow_smagorinsky", 1, "wavy_in_out", TF, turbulence_model=1, nut_initial=1e-5, les_ck=0.2)
add("pimple_through_flow_kEqn_linear_k_inlet", 1, "wavy_in_out", TF, k_convection_scheme=0, nut_bc=[3, 0, 3, 0], nut_val=[1e-5, 0, 1e-5, 0], **KEQN, **K_IN)
add("pimple_through_flow_kEqn_upwind_zeroGradient_relaxed", 1, "wavy_in_out", TF, k_convection_scheme=1, k_relax=0.9, **KEQN)      # inflow through a zeroGradient k patch
add("pimple_through_flow_kEqn_linear_zeroGradient_relaxed", 1, "wavy_in_out", TF, k_convection_scheme=0, k_relax=0.8, **KEQN)
add("pimple_through_flow_kEpsilon", 1, "wavy_in_out", TF, k_convection_scheme=1, eps_convection_scheme=0, eps_relax=0.8, **KEPS, **K_IN, **E_IN)
add("pimple_through_flow_kEpsilon_wall_functions", 1, "wavy_in_out", TF, k_convection_scheme=1, eps_convection_scheme=0, nut_bc=[0, 0, 2, 0], nut_val=[0.0] * 4,
    eps_bc=[1, 0, 2, 0], eps_val=[2e-3, 0, 1e-3, 0], **KEPS, **K_IN)
# (with k = 1e-4 the walls' y+ = Cmu^1/4 y sqrt(k) / nu is 3: nut_w = 0, the laminar branch.  The same with k = 8e-3, y+ 24 .. 27 above yPlusLam = 11.53: the logarithmic one)
add("pimple_through_flow_kEpsilon_wall_functions_log_layer", 1, "wavy_in_out", TF, k_convection_scheme=0, eps_convection_scheme=1, nut_bc=[0, 0, 2, 0], nut_val=[0.0] * 4,
    eps_bc=[1, 0, 2, 0], eps_val=[0.2, 0, 0.2, 0], k_bc=[1, 0, 0, 0], k_val=[8e-3, 0, 0, 0], **dict(KEPS, k_initial=8e-3, eps_initial=0.2, nut_initial=3e-5))
add("pimple_free_outlet_kEqn", 1, "wavy_in_out", through_flow(0.03, fixed_outlet=False), k_convection_scheme=0, **KEQN)            # adjustPhi acts

LAMINAR_SINGLE = [n for n, c in CASES.items() if not c["kw"].get("turbulence_model")]        # (the bit fixture's list)
SENSITIVITY = ("ico_wavy", "pimple_tetrahedra", "pimple_wavy_kEqn_linear", "pimple_through_flow_kEqn_linear_k_inlet")


# ---- the two sides' solvers --------------------------------------------------------------------------------------------------------------------------
def frozen(c):
    """the settings that freeze every count"""
    return dict(u_tol=0.0, u_rel_tol=0.0, u_max_iter=c["k_u"], p_tol=0.0, p_rel_tol=0.0, p_final_tol=0.0, p_final_rel_tol=0.0, p_max_iter=c["k_p"])


def expected_counts(c):
    """(u_iters_total, p_iters_total) of one step"""
    kw = c["kw"]
    n_outer = max(kw.get("n_outer", 1), 1) if c["solver"] == 1 else 1
    u = n_outer * c["k_u"] if kw.get("momentum_predictor", 1) else 0
    return u, n_outer * kw["n_correctors"] * (kw["n_non_orth"] + 1) * c["k_p"]


def counts_ok(c, stats):
    return (stats["u_iters_total"], stats["p_iters_total"]) == expected_counts(c)


PATCH_ARRAYS = ("u_bc", "u_val", "p_bc", "p_val", "nut_bc", "nut_val", "k_bc", "k_val", "eps_bc", "eps_val")


def _split(c, nu_factor=1.0):
    kw = dict(c["kw"], **frozen(c))
    dt, nu = kw.pop("dt"), kw.pop("nu") * nu_factor
    pos = [kw.pop("u_bc"), kw.pop("u_val"), kw.pop("p_bc"), kw.pop("p_val", None)]
    return dt, nu, pos, kw


def oracle_solver(orc, c, wide, nu_factor=1.0):
    dt, nu, pos, kw = _split(c, nu_factor)
    return orc.LduSolver(mesh_of(c), dt, nu, *pos, solver=c["solver"], wide=wide, **kw)


def product_solver(product, c):
    dt, nu, pos, kw = _split(c)
    patch = {k: kw.pop(k) for k in PATCH_ARRAYS if k in kw}
    if "n_outer" in kw:
        kw["n_outer_correctors"] = kw.pop("n_outer")
    return product.LduSolver(mesh_of(c), dt, nu, *pos, solver=c["solver"], p_solver=product.FY_PSOLVER_PCG_JACOBI, **patch, **kw)


def initial(c):
    """(U, p) the run starts from"""
    mesh = mesh_of(c)
    n = int(mesh["n_cells"])
    rs = np.random.RandomState(11)
    U = rs.rand(n, 3) * 0.05
    p = rs.rand(n) * 0.5
    if c["u0"] == "half_zero":                                  # (a hex_block: lattice cell i + nx (j + ny k) carries the number perm[...])
        nx = mesh["shape"][0]
        lat = np.arange(n)
        U[mesh["perm"][lat[lat % nx <= nx // 2]]] = 0.0
    return U, p


def external_source(c, step):
    """icoFoamYade's explicit momentum source of a step, or None"""
    if not c["source"]:
        return None
    return np.random.RandomState(51 + step).standard_normal((int(mesh_of(c)["n_cells"]), 3)) * 0.3


def records(c, step):
    """clustered particle records inside the mesh: drawn in the undistorted box, carried along by the vertex map (shear, waves, rotation)"""
    dims, _, vmap = MESHES[c["mesh"]]
    n, cluster = c["particles"]
    case = gc.Case("ldu_sweeps", *dims, dims[0] * H, gaussian=1, np_=n, seed=29, cluster=cluster, radius_dx=c["radius_dx"], vel_scale=0.05)
    rec = gc.particle_records(case, step)
    vm = vmap(box(dims))
    if vm is not None:
        rec[:, 0:3] = vm(rec[:, 0:3].copy())
    if c["mesh"] == "wavy_turned":
        rec[:, 3:6] = rec[:, 3:6] @ R.T
        rec[:, 6:9] = rec[:, 6:9] @ R.T
    return rec


def random_coupling(c, step):
    """seeded stand-ins of what the coupling leaves: alpha in [0.5, 1], a drag coefficient (<= 0: it is moved to the diagonal with its sign), a momentum source;
    icoFoamYade: the external source alone"""
    n = int(mesh_of(c)["n_cells"])
    rs = np.random.RandomState(101 + step)
    if c["solver"] == 1:
        return dict(alpha=0.5 + 0.5 * rs.rand(n), uSourceDrag=-50.0 * rs.rand(n), uSource=(rs.rand(n, 3) - 0.5) * 2.0)
    return dict(alpha=None, uSourceDrag=None, uSource=external_source(c, step))


# ---- which names a case compares ---------------------------------------------------------------------------------------------------------------------
def omitted(c):
    """{name: reason} over all names of GROUPS"""
    kw, out = c["kw"], dict(c["omit"])
    model, pimple = kw.get("turbulence_model", 0), c["solver"] == 1
    if model in (2, 3):
        for nm in ("HbyA", "mom_diag", "mom_b", "mom_lower", "mom_upper"):
            out[nm] = R_STORAGE
    if not pimple:
        for nm in ("gradP", "divT", "ddtU", "phiForces"):
            out[nm] = R_ICO
    if c["mesh"] != "cyclic":
        out["sep"] = R_NO_CYCLIC
    if not model:
        out["nut"] = R_NO_CLOSURE
    if model < 2:
        out["k"] = R_NO_K
    if model != 3:
        out["epsilon"] = R_NO_EPS
    assert not set(out) & set(NEVER_OMITTED), out
    return out


def compared(c):
    skip = omitted(c)
    return [nm for names in GROUPS.values() for nm in names if nm not in skip]


# ---- the oracle side -----------------------------------------------------------------------------------------------------------------------------------
def run_oracle(orc, c, coupling, wide, steps=2, names=None, nu_factor=1.0):
    """per step: ({name: field}, stats) of one build of the oracle, the coupling fields of `coupling[step]` handed to step() where setParticleAction stands"""
    o = oracle_solver(orc, c, wide, nu_factor)
    U0, p0 = initial(c)
    o.set("U", U0); o.set("p", p0)
    names, out = names or compared(c), []
    for step in range(steps):
        cpl = coupling[step]
        o.step(source=cpl["uSource"], alpha=cpl["alpha"], drag=cpl["uSourceDrag"])
        fields = {nm: (o.geometry(nm).ravel() if nm in GEOMETRY else o.get(oracle_name(c, nm))) for nm in names}
        if "kvec" in c["omit"]:
            assert np.abs(o.geometry("kvec")).max() < KVEC_NOISE
        out.append((fields, o.stats()))
    o.close()
    return out


BIT_NAMES = ("U", "p", "phi")


def oracle_bits(orc, name):
    """SHA-256 of U, p and phi after each of two steps of the double build (one thread, seeded random coupling fields): tests/golden/ldu_oracle_bits.json"""
    c = CASES[name]
    out = run_oracle(orc, c, [random_coupling(c, s) for s in range(2)], wide=False, names=BIT_NAMES)
    return [{nm: gc.sha(f[nm]) for nm in BIT_NAMES} for f, _ in out]


def distances(c, got, want):
    """{group: {name: distance}} of one step's (fields, stats) from the wide build's; the stats that follow phi go with it, and the time step as a field of one value"""
    (fa, sa), (fb, sb) = got, want
    out = {g: {} for g in GROUPS}
    for nm in fb:
        assert fa[nm].shape == fb[nm].shape, (nm, fa[nm].shape, fb[nm].shape)
        if not np.abs(fb[nm]).max() > 0:          # (a case names such a field in `zero`: tests/test_ldu_sweeps_reference.py)
            assert not np.abs(fa[nm]).max() > 0, f"{nm} is identically zero in the reference and is not here"
            continue
        out[GROUP_OF[nm]][nm] = rel(fa[nm], fb[nm])
    out["solved"]["courant_max"] = abs(sa["courant_max"] - sb["courant_max"]) / abs(sb["courant_max"])
    out["solved"]["cont_sum_local"] = abs(sa["cont_sum_local"] - sb["cont_sum_local"]) / cont_err_scale(c, fb, sb)
    out["solved"]["delta_t"] = abs(sa["delta_t"] - sb["delta_t"]) / abs(sb["delta_t"])
    return out


def cont_err_scale(c, fields, stats):
    """The unit in which sum local continuity error follows phi (fv_sweep_cases.cont_err_scale on a general mesh).  It is dt sum_cells |sum_faces phi| / V_total,
    the size of what the pressure solve leaves.  Faces that each move by e max |phi| move it by at most e times dt (2 internal + boundary faces) max |phi| /
    V_total (every face enters one or two cells' sums; alphacf <= 1): distances() divides by that, and the figure then lies under the bound of phi"""
    _, nf, ni = counts_of(mesh_of(c))
    return stats["delta_t"] * (nf + ni) * np.abs(fields["phi"]).max() / float(np.sum(fields["V"]))


class Envelope(fc.Envelope):
    """e_oracle per field group of this file and step (fv_sweep_cases.Envelope: the window, the bound, the report)"""

    def __init__(self):
        self.e = {(g, step): 0.0 for g in GROUPS for step in range(2)}
        self.at = dict.fromkeys(self.e, "-")
