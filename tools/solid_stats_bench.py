#!/usr/bin/env python
"""The solid-phase statistics at the benchmark size: the pass's kernel clock, and the coupled step with the statistics on against off.

    python tools/solid_stats_bench.py [--n 160] [--particles 10000000] [--steps 30] [--warmup 5] [--rounds 3] [--vel 0.1]

The case is bench.py's C3 (pimpleFoamYade, n^3 closed box, particles in the lower 60 %).  The statistics are switched on a solver (fy_solver_set_solid_statistics),
so two solvers of the same case -- one without, one with -- take `rounds` alternated legs of `steps` steps, each timed on the host around a device synchronisation.
Then one leg of the second solver with the per-kernel clocks on: "solid_stats" of fy_solver_get_kernel_timing is one event pair around all launches of the pass
(the clearing of the sums, two four-sum scatters with their tile reductions, the per-cell finish); the force pass of the same leg (fy_get_particle_timings) is the
yardstick.  --vel gives the particles velocities (the C3 cloud is at rest: the sums' values differ, the work does not).  Prints one JSON line."""
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
    ap.add_argument("--vel", type=float, default=0.0)
    args = ap.parse_args()
    import torch
    import bench
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda:0")
    rec = bench.c3_particles(torch, args.particles, args.n, 3, dev)
    if args.vel:
        rec[:, 3:6] = (torch.rand(args.particles, 3, dtype=torch.float64, device=dev) - 0.5) * 2 * args.vel

    def make(on):
        s = prod.Solver(bench.c3_case(prod, args.n, args.dt, 1))
        if on:
            s.set_solid_statistics(True)
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
    total, launches = s.kernel_timing("solid_stats")
    force_ms = s.coupling_timings()["force"]
    out = {"cells": args.n ** 3, "particles": args.particles, "solid_stats_ms": total / max(launches, 1), "solid_stats_samples": launches, "force_pass_ms": force_ms,
           "step_ms_off": ms[False], "step_ms_on": ms[True], "step_ms_difference": sum(ms[True]) / len(ms[True]) - sum(ms[False]) / len(ms[False])}
    print(json.dumps(out))
    for s in solvers.values():
        s.close()


if __name__ == "__main__":
    main()
