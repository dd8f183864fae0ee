"""The case list and the protocol that tests/test_fv_sweeps_reference.py (both builds of the CPU oracle) and tests/test_fv_sweeps_parity.py (the HIP solver) share:
the FV sweeps of the block solver -- fv_kernels.hip and the driver in fv_solver.cpp -- held to oracle/fv_oracle.cpp compiled in long double.

Protocol of a case.  Every iteration count is frozen (u_tol = u_rel_tol = 0 with u_max_iter = k_u; the pressure tolerances of tests/mg_cases.py with p_max_iter =
k_p; likewise k / epsilon), so a step is a fixed chain of operations and both sides can be held to rounding.  U (0 .. 0.05) and p start from seeded random
fields, two steps run.  The coupling fields alpha / uSource / uSourceDrag are written into the oracle between step_begin and step_end, in place of the particle
oracle: on the GPU they are the device's own (hold_sources keeps them readable after the step), so the FV halves of both sides see the same bits; without a
GPU they are seeded random fields.  The distance of a field is max |x - wide| / max |wide|.

Each case is there for the branch of a kernel or of the driver that it reaches; `omit` lists the names a case leaves out, with the reason."""
import numpy as np

import golden_cases as gc

FV, ZG, SLIP = 0, 1, 2            # velocity patch types
PZG, PFV, PFLUX = 0, 1, 2         # pressure patch types
XMIN, XMAX, YMIN, YMAX, ZMIN, ZMAX = range(6)
ADDED_MASS, GAUSSIAN_TORQUE = 1, 2

# ---- what is compared, by the point of the step at which it is final -------------------------------------------------------------------------------
GROUPS = {
    "assembled": ("gradP", "divT", "divG", "ddtU", "mom_diag", "mom_src", "rAU"),                     # before any solve of the momentum assembly that wrote them
    "predicted": ("HbyA", "p_diag", "p_ux", "p_uy", "p_uz", "p_rhs"),                                 # after the predictor
    "solved": ("U", "p", "phi_x", "phi_y", "phi_z", "vGrad", "nut", "k", "epsilon"),                  # after the pressure solve (and the closure's correct())
    # two diagnostics in groups of their own, so that what is noisy in them loosens no other bound: the neighbour coefficients of the momentum matrix (a limited
    # scheme's weight divides two differences of magSqr(U)) and the flux the pressure equation starts from (ddtCorr's coefficient divides by |phi|)
    "neighbours": tuple(f"mom_an{q}" for q in range(6)),
    "fluxHbyA": ("phiHbyA_x", "phiHbyA_y", "phiHbyA_z"),
}
GROUP_OF = {nm: grp for grp, names in GROUPS.items() for nm in names}
NEVER_OMITTED = ("U", "p", "phi_x", "phi_y", "phi_z", "rAU", "p_diag", "p_ux", "p_uy", "p_uz")
FACTOR = 50.0                                                # tests/test_mg_parity.py: contraction, summation order, single-reduction PCG, the Cholesky coarsest level
E_WINDOW = (1e-17, 1e-12)                                    # every group's e_oracle lies inside; the device bound can then never exceed 5e-11

R_STORAGE = "the device refuses it: kEqn / kEpsilon reuse the momentum matrix's storage after the last corrector"
R_ICO = "icoFoamYade forms neither (icoFoamYade.C:71 is grad(U) alone); the oracle's gradP is the corrector's, which the device never stores"
R_VGRAD = "the tiled stress sweep keeps grad(U) in LDS and nothing else asks for it"
R_DDTU = "ddtU_f is written for the added-mass model only"
R_NO_CLOSURE = "no turbulence model"
R_NO_EPS = "no epsilon equation"
R_NO_K = "no k equation"
R_DIVG = "icoFoamYade has no explicit stress term"
R_NO_CORRECTOR = "nCorrectors 0: no corrector runs, so nothing forms HbyA or assembles the pressure equation (its storage is whatever construction left)"
R_NO_ASSEMBLY = "one cell: the field is identically zero, a distance relative to its maximum does not exist"


def closed_box():
    """C3's boundary set: no-slip walls, fixedFluxPressure, gravity"""
    return dict(g=(0, 0, -9.81), u_bc=[FV] * 6, u_val=[(0, 0, 0)] * 6, p_bc=[PFLUX] * 6)


def c5_set(sides=FV):
    """C5's boundary set: z- inlet fixedValue, z+ outlet zeroGradient with p = 0, `sides` on x and y"""
    return dict(g=(0, 0, -9.81), u_bc=[sides] * 4 + [FV, ZG], u_val=[(0, 0, 0)] * 4 + [(0, 0, 0.05), (0, 0, 0)], p_bc=[PFLUX] * 5 + [PFV], p_val=[0.0] * 6)


def cavity(lid=1.0):
    u_val = [(0, 0, 0)] * 6
    u_val[YMAX] = (lid, 0, 0)
    return dict(u_bc=[FV] * 6, u_val=u_val, p_bc=[PZG] * 6)


def c2_channel():
    """C2's boundary set: x- inlet fixedValue, x+ outlet zeroGradient with p = 0, no-slip walls"""
    return dict(u_bc=[FV, ZG] + [FV] * 4, u_val=[(0.3, 0, 0)] + [(0, 0, 0)] * 5, p_bc=[PZG, PFV] + [PZG] * 4, p_val=[0.0] * 6)


def free_outlet():
    """no patch fixes the pressure and the outlet leaves U free: adjustPhi scales the outflow, the corrector takes its unfused front"""
    return dict(u_bc=[FV, ZG] + [FV] * 4, u_val=[(0.03, 0, 0)] + [(0, 0, 0)] * 5, p_bc=[PZG] * 6)


def sizes(n, ratio):
    """n cell sizes in geometric progression, last / first = ratio, summing to 0.1"""
    h = ratio ** (np.arange(n) / max(n - 1, 1))
    return h * (0.1 / h.sum())


def grading(dims):
    return (sizes(dims[0], 3.0), sizes(dims[1], 0.5), sizes(dims[2], 2.0))


SMALL, TILE_ODD, CLOSURE = (9, 7, 5), (19, 11, 7), (8, 8, 8)
CASES = {}


def add(name, solver, dims, bcs, couple=True, k_u=3, k_p=4, env=None, slabs=1, force_models=0, u0="random", graded=False, omit=None, zero=(), **kw):
    """kw: settings in the oracle's spelling (oracle.fv_case), shared by both sides"""
    assert name not in CASES
    kw = dict(bcs, **kw)
    if graded:
        kw["grading"] = grading(dims)
    kw.setdefault("p_solver", 1)
    kw.setdefault("u_relax", 1.0)
    # time step and viscosity put the three parts of the momentum matrix within an order of magnitude of each other (U up to 0.05, or the lid's 1, on cells of
    # 0.005 .. 0.01: Courant number and diffusion number 0.05 .. 0.2 beside the time derivative's 1), so that a defect in any of them shows; the closures keep a viscosity their nut can matter beside
    kw.setdefault("dt", 5e-3 if solver == 1 else 1e-3)
    kw.setdefault("nu", (1e-5 if kw.get("turbulence_model") else 2e-4) if solver == 1 else 0.01)
    CASES[name] = dict(name=name, solver=solver, dims=tuple(dims), couple=couple, k_u=k_u, k_p=k_p, env=dict(env or {}), slabs=slabs, force_models=force_models,
                       u0=u0, kw=kw, omit=dict(omit or {}), zero=tuple(zero))


SCHEMES = ("linear", "upwind", "linearUpwind", "limitedLinear", "vanLeer", "MUSCL", "Minmod", "SuperBee", "QUICK")
# ---- schemes: convection 0 .. 8, ico lid cavity and coupled pimple closed box; limitedLinear with k = 1 and 0.3
for q, nm in enumerate(SCHEMES):
    for solver, tag, bcs in ((0, "ico_cavity", cavity()), (1, "pimple_box", closed_box())):
        add(f"{tag}_{nm}", solver, SMALL, bcs, convection_scheme=q)
        if q == 3:
            add(f"{tag}_{nm}_k03", solver, SMALL, bcs, convection_scheme=q, limiter_k=0.3)
# the guard branches of the gradient ratio (NVDTVD::r): U uniform in half the box gives gradf = gradcf = 0 there and |gradcf| >= 1000 |gradf| beside it
add("ico_cavity_vanLeer_guard", 0, SMALL, cavity(), convection_scheme=4, u0="half_uniform")
add("pimple_box_limitedLinear_guard", 1, SMALL, closed_box(), convection_scheme=3, u0="half_uniform")
# ---- boundaries
add("pimple_c5", 1, SMALL, c5_set())
add("pimple_c5_slip_sides_QUICK", 1, SMALL, c5_set(SLIP), convection_scheme=8)
add("ico_c2_channel", 0, SMALL, c2_channel())
add("ico_free_outlet", 0, SMALL, free_outlet())
add("pimple_free_outlet", 1, SMALL, free_outlet())
# ---- the stress tile (16 x 8 x 4) and two-cells-per-thread indexing
add("pimple_box_19x11x7", 1, TILE_ODD, closed_box())
add("ico_cavity_19x11x7", 0, TILE_ODD, cavity())
add("pimple_box_16x8x4", 1, (16, 8, 4), closed_box())
# (one cell has no interior face and walls on x and y: its off-diagonal coefficients and the fluxes through x and y are identically zero on both sides, which
#  distances() demands exactly)
add("pimple_c5_1x1x1", 1, (1, 1, 1), c5_set(), couple=False, omit={"divG": R_NO_ASSEMBLY}, zero=("p_ux", "p_uy", "p_uz", "phi_x", "phi_y", "phiHbyA_x", "phiHbyA_y") + tuple(f"mom_an{q}" for q in range(6)))
# a plane of whole 256-cell blocks, 8 planes: the strip order of the cell sweeps is on.  (Jacobi-PCG: the strips reorder the FV sweeps, not the multigrid kernels,
#  and through the V-cycle of this closed 2048-cell box the double oracle itself lies 1e-12 from the wide one -- outside the window the bound rests on)
add("pimple_box_16x16x8_strips", 1, (16, 16, 8), closed_box(), p_solver=0)
# ---- graded blocks (ratios 3, 0.5, 2)
for q in (0, 1, 2, 4):
    add(f"pimple_graded_{SCHEMES[q]}", 1, TILE_ODD, closed_box(), graded=True, convection_scheme=q)
    add(f"ico_graded_{SCHEMES[q]}", 0, TILE_ODD, cavity(), graded=True, convection_scheme=q)
add("pimple_graded_c5_slip_sides", 1, TILE_ODD, c5_set(SLIP), graded=True)
# ---- closures
KEQN = dict(turbulence_model=2, k_initial=1e-4, nut_initial=1e-5, k_tol=0.0, k_rel_tol=0.0, k_max_iter=3)
KEPS = dict(turbulence_model=3, k_initial=1e-4, eps_initial=1e-3, nut_initial=1e-5, k_tol=0.0, k_rel_tol=0.0, k_max_iter=3, eps_tol=0.0, eps_rel_tol=0.0, eps_max_iter=3)
WALLS = dict(nut_bc=[2] * 6, nut_value=[0.0] * 6, eps_bc=[2] * 6, eps_value=[1e-3] * 6, k_bc=[0] * 6)
add("pimple_smagorinsky", 1, CLOSURE, closed_box(), turbulence_model=1, nut_initial=1e-5, les_ck=0.2)
add("pimple_smagorinsky_outer2", 1, CLOSURE, closed_box(), turbulence_model=1, nut_initial=1e-5, n_outer=2, u_relax=0.9)
add("pimple_kEqn_linear", 1, CLOSURE, closed_box(), k_convection_scheme=0, **KEQN)
add("pimple_kEqn_upwind", 1, CLOSURE, closed_box(), k_convection_scheme=1, **KEQN)
add("pimple_kEpsilon", 1, CLOSURE, closed_box(), **KEPS)
add("pimple_kEpsilon_wall_functions", 1, CLOSURE, closed_box(), **dict(KEPS, **WALLS))
add("pimple_graded_smagorinsky", 1, TILE_ODD, closed_box(), graded=True, turbulence_model=1, nut_initial=1e-5)
# ---- closures on sides that carry a flux.  In a closed box the transport sweeps (k_assemble_turb / k_turb_finish, the oracle's turb_eqn) never see the boundary
# convection term, the negative diagonal contribution of inflow through a zeroGradient patch (and fvMatrix::relax's dominance test with it), a divU in SuSp that
# is not the pressure solve's residual, bound()'s face average at a fixed-value patch, or a wall-function cell beside an inlet.  Every case names its k (and
# epsilon) scheme: fy_case_defaults says upwind, fy_ldu_case_defaults linear, and a case that leaves it open compares two different equations across solvers
K_IN = dict(k_bc=[0, 0, 0, 0, 1, 0], k_value=[0, 0, 0, 0, 2e-4, 0])
E_IN = dict(eps_bc=[0, 0, 0, 0, 1, 0], eps_value=[0, 0, 0, 0, 2e-3, 0])
WALLS_C5 = dict(nut_bc=[2] * 4 + [0, 0], nut_value=[0.0] * 6, eps_bc=[2] * 4 + [1, 0], eps_value=[1e-3] * 4 + [2e-3, 0])       # wall-function sides, inlet, outlet
add("pimple_c5_smagorinsky", 1, CLOSURE, c5_set(), turbulence_model=1, nut_initial=1e-5, les_ck=0.2)
add("pimple_c5_kEqn_linear_k_inlet", 1, CLOSURE, c5_set(), k_convection_scheme=0, **KEQN, **K_IN)
add("pimple_c5_kEqn_upwind_zeroGradient_relaxed", 1, CLOSURE, c5_set(), k_convection_scheme=1, k_relax=0.9, **KEQN)      # inflow through a zeroGradient k patch
add("pimple_c5_kEqn_linear_zeroGradient_relaxed", 1, CLOSURE, c5_set(), k_convection_scheme=0, k_relax=0.8, **KEQN)
add("pimple_c5_slip_kEqn_calculated_nut", 1, CLOSURE, c5_set(SLIP), k_convection_scheme=0, nut_bc=[3] * 6, nut_value=[2e-5] * 6, **KEQN, **K_IN)
add("pimple_c5_kEpsilon_inlet", 1, CLOSURE, c5_set(), k_convection_scheme=1, eps_convection_scheme=0, eps_relax=0.8, **KEPS, **K_IN, **E_IN)
add("pimple_c5_kEpsilon_wall_functions", 1, CLOSURE, c5_set(), k_convection_scheme=1, eps_convection_scheme=0, **KEPS, **K_IN, **WALLS_C5)
# (with k = 1e-4 the walls' y+ = Cmu^1/4 y sqrt(k) / nu is 3.4: nut_w = 0, the laminar branch.  The same with k = 8e-3, y+ 30 above yPlusLam = 11.53: the logarithmic one)
add("pimple_c5_kEpsilon_wall_functions_log_layer", 1, CLOSURE, c5_set(), k_convection_scheme=0, eps_convection_scheme=1, k_bc=K_IN["k_bc"], k_value=[0, 0, 0, 0, 8e-3, 0],
    **dict(KEPS, k_initial=8e-3, eps_initial=0.2, nut_initial=3e-5), **dict(WALLS_C5, eps_value=[0.2] * 6))
add("pimple_free_outlet_kEqn", 1, CLOSURE, dict(free_outlet(), g=(0, 0, -9.81)), k_convection_scheme=0, **KEQN)           # adjustPhi acts; the inlet's k is zeroGradient
add("pimple_graded_c5_kEqn", 1, TILE_ODD, c5_set(), graded=True, k_convection_scheme=0, **KEQN, **K_IN)
add("pimple_graded_c5_kEpsilon_wall_functions", 1, TILE_ODD, c5_set(), graded=True, k_convection_scheme=1, eps_convection_scheme=1, **KEPS, **K_IN, **WALLS_C5)
# (two z-slabs, held to the single-domain reference: the inlet belongs to the first slab and the outlet to the last)
add("pimple_c5_19x11x12_kEqn_slabs2", 1, (19, 11, 12), c5_set(), slabs=2, k_convection_scheme=0, **KEQN, **K_IN)
# ---- driver branches
for solver, tag, bcs in ((0, "ico_cavity", cavity()), (1, "pimple_box", closed_box())):
    for n_outer, n_corr, n_no in ((1, 1, 0), (1, 2, 0), (1, 3, 1), (2, 1, 0), (3, 2, 0)):
        if solver == 0 and n_outer > 1:
            continue                                                            # (icoFoamYade has no outer loop)
        add(f"{tag}_loops_{n_outer}{n_corr}{n_no}", solver, SMALL, bcs, n_outer=n_outer, n_corr=n_corr, n_non_orth=n_no)
    add(f"{tag}_no_predictor", solver, SMALL, bcs, momentum_predictor=0)
    add(f"{tag}_no_predictor_non_orth", solver, SMALL, bcs, momentum_predictor=0, n_non_orth=1)
    for k_u in (0, 1):                                                          # (3: every other case) the predictor's pass hands HbyA to the corrector from its second pass on
        add(f"{tag}_ku{k_u}", solver, SMALL, bcs, k_u=k_u)
    add(f"{tag}_unfused_corrector", solver, SMALL, bcs, env={"FOAMYADE_NO_FUSED_CORRECTOR": "1"})
    add(f"{tag}_no_correctors", solver, SMALL, bcs, n_corr=0, omit={nm: R_NO_CORRECTOR for nm in GROUPS["predicted"] + GROUPS["fluxHbyA"]})      # the flux takes the copy branch of step()
    add(f"{tag}_jacobi_pcg", solver, SMALL, bcs, p_solver=0)
add("pimple_box_relaxation", 1, SMALL, closed_box(), n_outer=2, u_relax=0.7, p_relax=0.3, p_relax_final=1.0)
add("pimple_box_adjust_time_step", 1, SMALL, closed_box(), adjust_time_step=1, max_co=0.02, max_delta_t=0.1)
add("pimple_box_force_models", 1, SMALL, closed_box(), force_models=ADDED_MASS | GAUSSIAN_TORQUE)
# ---- kernel switches, each held to the reference (not to the default path)
SWITCHES = ({"FOAMYADE_NO_FUSED_CORRECTOR": "1"}, {"FOAMYADE_FACES_FROM_ARRAYS": "1"}, {"FOAMYADE_STRIP_BLOCKS": "0"}, {"FOAMYADE_STRIP_BLOCKS": "1"},
            {"FOAMYADE_NO_TILED_STRESS": "1"}, {"FOAMYADE_NO_PAIRS": "1"}, {"FOAMYADE_NO_TAIL_CACHE": "1"})
for env in SWITCHES:
    (sw, val), = env.items()
    tag = sw[len("FOAMYADE_"):].lower() + ("" if val == "1" and "STRIP" not in sw else val)
    add(f"pimple_box_19x11x7_{tag}", 1, TILE_ODD, closed_box(), env=env)
    add(f"ico_cavity_19x11x7_{tag}", 0, TILE_ODD, cavity(), env=env)
add("pimple_box_16x16x8_strip_blocks0", 1, (16, 16, 8), closed_box(), p_solver=0, env={"FOAMYADE_STRIP_BLOCKS": "0"})
# ---- z-slabs (VirtualSlabs), held to the single-domain reference
# (a pimpleFoamYade slab carries the five ghost planes of the Gaussian stencil and an even number of planes: three slabs need nz = 18)
for n, nz in ((2, 12), (3, 18)):
    add(f"pimple_box_19x11x{nz}_slabs{n}", 1, (19, 11, nz), closed_box(), slabs=n)
    add(f"ico_cavity_19x11x12_slabs{n}", 0, (19, 11, 12), cavity(), slabs=n)

LAMINAR_SINGLE = [n for n, c in CASES.items() if not c["kw"].get("turbulence_model") and not c["env"] and c["slabs"] == 1]       # (the bit fixture's list)


# ---- the two sides' case objects -----------------------------------------------------------------------------------------------------------------------
def dx_of(c):
    return 0.1 / max(c["dims"])


def frozen(c):
    """the settings that freeze every count"""
    return dict(u_tol=0.0, u_rel_tol=0.0, u_max_iter=c["k_u"], p_tol=1e-30, p_final_tol=1e-30, p_rel_tol=0.0, p_final_rel_tol=0.0, p_max_iter=c["k_p"])


def counts_ok(c, stats):
    """u_iters_total and p_iters_total of a step are the frozen ones.  The one-cell block is the exception the protocol cannot freeze: PCG solves one equation
    exactly in its first iteration, the residual is then zero (or one rounding of it) and the solve ends -- as it must, the next iteration would divide 0 by 0"""
    u, p = expected_counts(c)
    if int(np.prod(c["dims"])) == 1:
        return stats["u_iters_total"] == u and 1 <= stats["p_iters_total"] <= p
    return (stats["u_iters_total"], stats["p_iters_total"]) == (u, p)


def expected_counts(c):
    """(u_iters_total, p_iters_total) of one step"""
    kw = c["kw"]
    n_outer = max(kw.get("n_outer", 1), 1) if c["solver"] == 1 else 1
    u = n_outer * c["k_u"] if kw.get("momentum_predictor", 1) else 0
    return u, n_outer * kw.get("n_corr", 2) * (kw.get("n_non_orth", 0) + 1) * c["k_p"]


def oracle_case(orc, c):
    kw = dict(c["kw"], **frozen(c))
    dt, nu = kw.pop("dt"), kw.pop("nu")
    return orc.fv_case(c["solver"], *c["dims"], dx_of(c), dt, nu, **kw)


PRODUCT_NAMES = {"n_outer": "n_outer_correctors", "n_corr": "n_correctors", "n_non_orth": "n_non_orth_correctors", "limiter_k": "convection_limiter_k"}


def product_case(product, c):
    kw = {PRODUCT_NAMES.get(k, k): v for k, v in dict(c["kw"], **frozen(c)).items()}
    dt, nu = kw.pop("dt"), kw.pop("nu")
    return product.make_case(c["solver"], *c["dims"], dx_of(c), dt, nu, **kw)


def initial(c):
    """(U, p) the run starts from"""
    nx, ny, nz = c["dims"]
    rs = np.random.RandomState(11)
    U = rs.rand(nz, ny, nx, 3) * 0.05
    p = rs.rand(nz * ny * nx) * 0.5
    if c["u0"] == "half_uniform":
        U[:, :, : nx // 2 + 1] = (0.02, 0.01, 0.015)
    return U.reshape(-1, 3), p


def records(c, step):
    """a few hundred clustered particle records inside the block (the 0.1-long block of the graded cases is not one of cubes: a 10^3 stand-in of its extent)"""
    nx, ny, nz = c["dims"]
    shape = (10, 10, 10) if "grading" in c["kw"] else (nx, ny, nz)
    case = gc.Case("fv_sweeps", *shape, shape[0] * (0.01 if "grading" in c["kw"] else dx_of(c)), gaussian=c["solver"], np_=300, seed=29, cluster=80, radius_dx=0.3, vel_scale=0.05)
    return gc.particle_records(case, step)


def random_coupling(c, step):
    """seeded stand-ins of what the coupling leaves: alpha in [0.5, 1], a drag coefficient (<= 0: it is moved to the diagonal with its sign), a momentum source"""
    n = int(np.prod(c["dims"]))
    rs = np.random.RandomState(101 + step)
    if c["solver"] == 1:
        return dict(alpha=0.5 + 0.5 * rs.rand(n), uSourceDrag=-50.0 * rs.rand(n), uSource=(rs.rand(n, 3) - 0.5) * 2.0)
    return dict(alpha=np.ones(n), uSourceDrag=np.zeros(n), uSource=(rs.rand(n, 3) - 0.5) * 2.0)


def no_coupling(c):
    n = int(np.prod(c["dims"]))
    return dict(alpha=np.ones(n), uSourceDrag=np.zeros(n), uSource=np.zeros((n, 3)))


# ---- which names a case compares ---------------------------------------------------------------------------------------------------------------------
def omitted(c):
    """{name: reason} over all names of GROUPS"""
    kw, out = c["kw"], dict(c["omit"])
    model, pimple = kw.get("turbulence_model", 0), c["solver"] == 1
    if model in (2, 3):
        for nm in ("HbyA", "mom_diag", "mom_src") + tuple(f"mom_an{q}" for q in range(6)):
            out[nm] = R_STORAGE
    if not pimple:
        out.update(gradP=R_ICO, divT=R_ICO, divG=R_DIVG)
    # grad(U) is stored by icoFoamYade's opening sweep, for the Gaussian torque, by the two stress sweeps of linearUpwind, and by the closure's correct()
    stored = not pimple or model or (c["force_models"] & GAUSSIAN_TORQUE) or kw.get("convection_scheme", 0) == 2
    if not stored:
        out["vGrad"] = R_VGRAD
    if not (c["force_models"] & ADDED_MASS):
        out["ddtU"] = R_DDTU
    if not model:
        out["nut"] = R_NO_CLOSURE
    if model < 2:
        out["k"] = R_NO_K
    if model != 3:
        out["epsilon"] = R_NO_EPS
    never = [nm for nm in NEVER_OMITTED if kw.get("n_corr", 2) > 0 or GROUP_OF[nm] != "predicted"]
    assert not set(out) & set(never), out
    return out


def compared(c):
    skip = omitted(c)
    return [nm for names in GROUPS.values() for nm in names if nm not in skip]


# ---- the oracle side -----------------------------------------------------------------------------------------------------------------------------------
def run_oracle(orc, c, coupling, wide, steps=2, names=None):
    """per step: ({name: field}, stats) of one build of the oracle, the coupling fields of `coupling[step]` written in where setParticleAction stands"""
    o = orc.FvSolver(oracle_case(orc, c), wide=wide)
    U0, p0 = initial(c)
    o.set("U", U0); o.set("p", p0)
    names, out = names or compared(c), []
    for step in range(steps):
        o.step_fields(coupling[step])
        out.append(({nm: o.get(nm) for nm in names}, o.stats()))
    o.close()
    return out


BIT_NAMES = ("U", "p", "phi_x", "phi_y", "phi_z")


def oracle_bits(orc, name):
    """SHA-256 of U, p and phi_* after each of two steps of the double build (one thread, seeded random coupling fields): tests/golden/fv_oracle_bits.json"""
    c = CASES[name]
    out = run_oracle(orc, c, [random_coupling(c, s) if c["couple"] else no_coupling(c) for s in range(2)], wide=False, names=BIT_NAMES)
    return [{nm: gc.sha(f[nm]) for nm in BIT_NAMES} for f, _ in out]


def rel(a, ref):
    """max |a - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def distances(c, got, want):
    """{group: {name: distance}} of one step's (fields, stats) from the wide build's; the two stats that follow phi go with it"""
    (fa, sa), (fb, sb) = got, want
    cont_scale = cont_err_scale(c, fb, sb)
    out = {g: {} for g in GROUPS}
    for nm in fb:
        assert fa[nm].shape == fb[nm].shape, nm
        if not np.abs(fb[nm]).max() > 0:          # (a case names such a field in `zero`: tests/test_fv_sweeps_reference.py)
            assert not np.abs(fa[nm]).max() > 0, f"{nm} is identically zero in the reference and is not here"
            continue
        out[GROUP_OF[nm]][nm] = rel(fa[nm], fb[nm])
    out["solved"]["courant_max"] = abs(sa["courant_max"] - sb["courant_max"]) / abs(sb["courant_max"])
    out["solved"]["cont_sum_local"] = abs(sa["cont_sum_local"] - sb["cont_sum_local"]) / cont_scale
    return out


def cont_err_scale(c, fields, stats):
    """The unit in which sum local continuity error follows phi.  It is dt sum_cells |sum_faces phi| / V_total, the size of what the pressure solve leaves --
    rounding noise once the solve has converged, so a distance relative to itself would say nothing.  Faces that each move by e max |phi| move it by at most
    e times dt 6 N_cells max |phi| / V_total: distances() divides by that, and the figure then lies under the bound of phi"""
    n = int(np.prod(c["dims"]))
    vol = float(np.prod([np.sum(h) for h in c["kw"]["grading"]])) if "grading" in c["kw"] else n * dx_of(c) ** 3
    return stats["delta_t"] * 6.0 * n * max(np.abs(fields[nm]).max() for nm in ("phi_x", "phi_y", "phi_z")) / vol


class Envelope:
    """e_oracle: per field group and step, the largest distance of the double build from the wide one over the case list.  (Per step because the second step's
    figures carry the first step's pressure solve: the first step's bound on what is assembled before any solve stays at a few ulp.)"""

    def __init__(self):
        self.e = {(g, step): 0.0 for g in GROUPS for step in range(2)}
        self.at = dict.fromkeys(self.e, "-")

    def add(self, name, step, per_group):
        w = worst(per_group)
        for g, (v, nm) in w.items():
            if v > self.e[(g, step)]:
                self.e[(g, step)], self.at[(g, step)] = v, f"{nm} of {name}"
        return w

    def check_window(self):
        for k, v in self.e.items():
            assert E_WINDOW[0] < v < E_WINDOW[1], (k, v, self.at[k])

    def bound(self, g, step):
        """what the device gets"""
        return FACTOR * max(self.e[(g, step)], 2.0 ** -52)

    def report(self, title="e_oracle"):
        return "\n".join(f"{title} {g:9s} step {step + 1}: {v:.2e}  ({self.at[(g, step)]})" for (g, step), v in self.e.items())


def worst(per_group):
    """{group: (largest distance, its name)}"""
    return {g: max(((v, nm) for nm, v in d.items()), default=(0.0, "-")) for g, d in per_group.items()}
