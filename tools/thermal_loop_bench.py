#!/usr/bin/env python
"""The particle passes of the heat exchange with and without the thermal loop: their kernel clocks on a pimpleFoamYade block.

    python tools/thermal_loop_bench.py [--n 64] [--particles 1000000] [--steps 10] [--warmup 3] [--particle-cp 0] [--beta 0] [--t-ref 300]

The case is bench.py's C3 at the given size (closed box, particles at rest in the lower 60 %) with water's cp and kappa, the fluid at 300 K and the particles at 350 K.
After `warmup` steps the kernel clocks are switched on (which resets them) and `steps` steps are timed: "heat_coeff" (pass A), "heat_flux" (pass B) and, with beta != 0,
"buoyancy" of fy_solver_get_kernel_timing, each as milliseconds per step.  The new descriptor fields are only touched when they are non-zero, so the same file measures
a tree from before they existed (particle_cp = beta = 0 there).  One process, one measurement: comparisons alternate processes of the two trees.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1e-4)
    ap.add_argument("--particle-cp", type=float, default=0.0)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--t-ref", type=float, default=300.0)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    import bench
    from __graft_entry__ import load_product
    prod = load_product()
    rec = bench.c3_particles(torch, args.particles, args.n, 3, torch.device("cuda:0"))
    case = bench.c3_case(prod, args.n, args.dt, 1)
    loop = {}
    if args.particle_cp:
        loop["particle_cp"] = args.particle_cp
    if args.beta:
        loop.update(beta=args.beta, T_ref=args.t_ref)
    case.thermal = prod.thermal_desc(4180.0, 0.6, T_initial=300.0, particle_temperature=350.0, T_tol=1e-8, T_max_iter=50, **loop)
    s = prod.Solver(case)
    s.set_particles_device(rec)
    for _ in range(args.warmup):
        s.step()
    s.enable_kernel_timing(True)
    for _ in range(args.steps):
        s.step()
    torch.cuda.synchronize()
    out = {"label": args.label, "cells": args.n ** 3, "particles": args.particles, "particle_cp": args.particle_cp, "beta": args.beta, "steps": args.steps}
    for name in ("heat_coeff", "heat_flux") + (("buoyancy",) if args.beta else ()):
        total, launches = s.kernel_timing(name)
        out[name + "_ms"] = total / max(launches, 1)
    out["heat_to_particles_W"] = s.thermal_stats()[2]
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
