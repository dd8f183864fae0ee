#!/usr/bin/env python
"""Heat exchange at the benchmark size: its three kernel clocks, and the coupled step with thermal on against off.

    python tools/heat_transfer_bench.py [--n 160] [--particles 10000000] [--steps 30] [--warmup 5] [--rounds 3] [--law RanzMarshall|Gunn]

The case is bench.py's C3 (pimpleFoamYade, n^3 closed box, particles at rest in the lower 60 %) with water's cp and kappa, the fluid at 300 K and the particles
at 350 K.  Thermal is a property of the case a solver is made from, so two solvers -- one without, one with -- take `rounds` alternated legs of `steps` steps,
each timed on the host around a device synchronisation.  Then one leg of the thermal solver with the per-kernel clocks on: "heat_coeff" (pass A: coefficients,
the LDS-aggregated scatter and the tile reduction), "T_assemble" (k_assemble_scalar) and "heat_flux" (pass B) of fy_solver_get_kernel_timing, each an event pair
around the phase's launches; the force pass of the same leg (fy_get_particle_timings) is the yardstick for the two particle passes.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1e-4)
    ap.add_argument("--law", default="RanzMarshall", choices=["RanzMarshall", "Gunn"])
    args = ap.parse_args()
    import torch
    import bench
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda:0")
    rec = bench.c3_particles(torch, args.particles, args.n, 3, dev)

    def make(on):
        case = bench.c3_case(prod, args.n, args.dt, 1)
        if on:
            case.thermal = prod.thermal_desc(4180.0, 0.6, T_initial=300.0, particle_temperature=350.0, T_tol=1e-8, T_max_iter=50,
                                             nusselt_law=prod.NUSSELT_GUNN if args.law == "Gunn" else prod.NUSSELT_RANZ_MARSHALL)
        s = prod.Solver(case)
        s.set_particles_device(rec)
        return s

    solvers = {False: make(False), True: make(True)}

    def leg(s, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for s in solvers.values():
        leg(s, args.warmup)
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            ms[on].append(leg(solvers[on], args.steps))
    s = solvers[True]
    s.enable_kernel_timing(True)
    s.enable_particle_timing(True)
    leg(s, args.steps)
    clocks = {}
    for name in ("heat_coeff", "T_assemble", "heat_flux"):
        total, launches = s.kernel_timing(name)
        clocks[name + "_ms"] = total / max(launches, 1)
    force_ms = s.coupling_timings()["force"]
    iters, res0, heat = s.thermal_stats()
    out = {"cells": args.n ** 3, "particles": args.particles, "law": args.law, **clocks, "force_pass_ms": force_ms, "T_passes": iters, "T_initial_residual": res0,
           "heat_to_particles_W": heat, "step_ms_off": ms[False], "step_ms_on": ms[True], "step_ms_difference": sum(ms[True]) / len(ms[True]) - sum(ms[False]) / len(ms[False])}
    print(json.dumps(out))
    for s in solvers.values():
        s.close()


if __name__ == "__main__":
    main()
