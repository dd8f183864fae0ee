#!/usr/bin/env python3
"""fy_ldu_solver (icoFoamYade on a general polyhedral mesh, LDU addressing) at scale: a lid-driven cavity on n^3 hexahedra written as a polyhedral mesh,
plain and wavy (non-orthogonal + skewed, one non-orthogonal corrector), against the structured fy_solver on the same lattice.
usage: ldu_bench.py [n=128] [steps=10] [kind=wavy|lattice|prisms] [particles=0] [p_solver=mg|diag] [nu=1e-4] [solver=ico|pimple] [turb=laminar|kEpsilon|kEpsilonWF]
             [--thermal] [--particle-cp=C] [--beta=B] [--flow-control]                                                               -> one JSON line
pimple: a closed box under gravity (fixedFluxPressure walls), the cloud at rest in its lower 60 %, Gaussian 4-way coupling; turb (pimple only): RAS kEpsilon with
zero-gradient k / epsilon / nut patches, or kEpsilonWF: with nutkWallFunction / epsilonWallFunction on every side of the box.
--thermal: the fluid temperature equation and the particle-fluid heat exchange (fy_ldu_case.thermal) with water's cp and kappa, the fluid at 300 K and the particles
at 350 K, zeroGradient T patches (tools/thermal_loop_bench.py's case); --particle-cp: the library integrates the particle temperatures; --beta: Boussinesq buoyancy
about 300 K (it needs gravity: solver=pimple).  The output then carries the T solve's Jacobi passes of the last step and the heat the particles received in the last step.
--flow-control: flow-rate control (fy_ldu_case.flow_control) holding Ubar = (0.1 0 0) with relaxation 1, its kernels timed one by one: the output carries the
"flow_control" clock per step and per launch, and the last correction's numbers"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import __graft_entry__ as ge  # noqa: E402
import poly_meshes as pm  # noqa: E402

flags = {a.split("=")[0]: (a.split("=") + [""])[1] for a in sys.argv[1:] if a.startswith("--")}
sys.argv = [a for a in sys.argv if not a.startswith("--")]
if set(flags) - {"--thermal", "--particle-cp", "--beta", "--flow-control"}:
    sys.exit("flags: --thermal [--particle-cp=C] [--beta=B] [--flow-control]")
flow_on = "--flow-control" in flags
thermal_on = "--thermal" in flags
n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
kind = sys.argv[3] if len(sys.argv) > 3 else "wavy"
npart = int(sys.argv[4]) if len(sys.argv) > 4 else 0
psolver = sys.argv[5] if len(sys.argv) > 5 else "mg"
nu = float(sys.argv[6]) if len(sys.argv) > 6 else 1e-4
solver = sys.argv[7] if len(sys.argv) > 7 else "ico"
turb = sys.argv[8] if len(sys.argv) > 8 else "laminar"
pimple = solver == "pimple"
if turb not in ("laminar", "kEpsilon", "kEpsilonWF") or (turb != "laminar" and not pimple):
    sys.exit("turb: laminar | kEpsilon | kEpsilonWF (the last two with solver=pimple)")
prod = ge.load_product()
L = 0.1
t0 = time.time()
vm = None if kind == "lattice" else pm.wavy(0.15 * L / n * 4, (L, L, L))
mesh = pm.prism_block(n, n, max(n // 2, 1), (L, L, L), vm) if kind == "prisms" else pm.hex_block_fast(n, n, n, (L, L, L), vm)
t_mesh = time.time() - t0
lid = [(0, 0, 0)] * 6
lid[3] = (1.0, 0, 0)
dt = 0.2 * (L / n) / 1.0
kw = dict(n_non_orth=0 if kind == "lattice" else 1, p_tol=1e-6, p_rel_tol=0.05, p_final_tol=1e-6, u_tol=1e-5, p_max_iter=2000,
          p_solver=prod.FY_PSOLVER_PCG_MG if psolver == "mg" else prod.FY_PSOLVER_PCG_JACOBI)
if thermal_on:
    loop = {}
    if flags.get("--particle-cp"):
        loop["particle_cp"] = float(flags["--particle-cp"])
    if flags.get("--beta"):
        loop.update(beta=float(flags["--beta"]), T_ref=300.0)
    kw["thermal"] = prod.thermal_desc(4180.0, 0.6, T_initial=300.0, particle_temperature=350.0, T_tol=1e-8, T_max_iter=50, **loop)
if flow_on:
    kw["flow_control"] = prod.flow_control_desc((0.1, 0.0, 0.0))
t0 = time.time()
if pimple:
    dt = 1e-4
    kw.update(solver=1, g=(0.0, 0.0, -9.81), n_outer_correctors=1, u_relax=1.0)
    if turb != "laminar":
        kw.update(turbulence_model=prod.TURBULENCE_KEPSILON, nut_initial=9e-6, k_initial=1e-4, eps_initial=1e-4, k_tol=1e-8, eps_tol=1e-8)
        if turb == "kEpsilonWF":
            kw.update(nut_bc=[prod.BC_WALL_FUNCTION] * 6, eps_bc=[prod.BC_WALL_FUNCTION] * 6)
    s = prod.LduSolver(mesh, dt, 1e-6, [0] * 6, [(0, 0, 0)] * 6, [2] * 6, **kw)
else:
    s = prod.LduSolver(mesh, dt, nu, [0] * 6, lid, [0] * 6, **kw)
t_create = time.time() - t0
if npart:
    rs = np.random.RandomState(5)
    rec = np.zeros((npart, 10))
    rec[:, 0:3] = L * (0.1 + 0.8 * rs.rand(npart, 3)); rec[:, 9] = 1e-5 + 0.5e-5 * rs.rand(npart)          # (radius)
    if pimple:
        rec[:, 0:3] = L * rs.rand(npart, 3) * np.array([1.0, 1.0, 0.6]); rec[:, 9] = 0.2 * L / n
    s.set_particles(rec)
for _ in range(3):
    s.step()
if flow_on:
    s.enable_kernel_timing(True)
its = uits = 0
ms = mp = 0.0
t0 = time.time()
for _ in range(steps):
    s.step()
    st = s.stats()
    its += st["p_iters_total"]; uits += st["u_iters_total"]; ms += st["ms_total"]; mp += st["ms_particle"]
wall = time.time() - t0
out = dict(tool="ldu_bench", kind=kind, turb=turb, cells=int(mesh["n_cells"]), faces=int(len(mesh["owner"])), steps=steps, steps_per_s=steps / wall, ms_per_step_wall=1e3 * wall / steps,
           ms_per_step_stream=ms / steps, ms_particle=mp / steps, solver=solver, pcg_iters_per_step=its / steps, p_solver=psolver, nu=nu, u_sweeps_per_step=uits / steps, us_per_pcg_iter=1e3 * ms / max(its, 1), courant_max=st["courant_max"],
           cont_err=st["cont_err_sum_local"], particles=npart, mesh_build_s=t_mesh, create_s=t_create, non_orth=kw["n_non_orth"])
if thermal_on:
    out.update(thermal=True, particle_cp=float(flags.get("--particle-cp") or 0), beta=float(flags.get("--beta") or 0), T_passes_last_step=s.thermal_stats()[0],
               heat_to_particles_W=s.thermal_stats()[2] if npart else 0.0)
if flow_on:
    fms, fl = s.kernel_timing("flow_control")
    out.update(flow_control=s.flow_control(), flow_control_ms_per_step=fms / steps, flow_control_launches_per_step=fl / steps, flow_control_us_per_launch=1e3 * fms / max(fl, 1))
s.close()
if kind == "lattice" and n % 8 == 0:
    # the structured solver on the same block with the same controls (PCG + diagonal preconditioner)
    c = prod.make_case(prod.FY_SOLVER_ICO, n, n, n, L / n, dt, nu, u_val=lid, p_tol=1e-6, p_rel_tol=0.05, p_final_tol=1e-6, u_tol=1e-5, p_max_iter=2000,
                       p_solver=prod.FY_PSOLVER_PCG_MG if psolver == "mg" else prod.FY_PSOLVER_PCG_JACOBI)
    h = prod.Solver(c)
    for _ in range(3):
        h.step()
    t0 = time.time(); its2 = 0
    for _ in range(steps):
        h.step(); its2 += h.stats()["p_iters_total"]
    w2 = time.time() - t0
    out.update(structured_ms_per_step=1e3 * w2 / steps, structured_pcg_iters_per_step=its2 / steps)
    h.close()
print(json.dumps(out))
