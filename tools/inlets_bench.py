#!/usr/bin/env python
"""Inlets at the benchmark size: the update kernel's time on its own clock, and the coupled step with a full-side per-face inlet against the same run with a uniform inlet.

    python tools/inlets_bench.py [--n 160] [--particles 10000000] [--steps 30] [--warmup 5] [--rounds 3]

The case is bench.py's C3 box and cloud (pimpleFoamYade, n^3 cells, particles at rest in the lower 60 %) opened for a through-flow: the bottom side z- is a fixed-value
inlet, the top side z+ lets U float at a fixed pressure, the four walls stay as they are.  Two solvers with the same cloud: A carries the uniform value v on z-, B an inlet
over all n^2 faces of z- whose per-face shape is v on every face, scaled by a table that stays at 1 -- the same flow, so the two step the same work and differ only in
where a boundary value comes from (the update kernel, and the per-face loads in the sweeps).  The legs alternate, `rounds` times each, `steps` steps per leg timed on the
host around a device synchronisation.  Then a third solver repeats A's steps: what the two flows differ by is printed beside what two runs of the same case differ by (the cloud's scatter is a sum of
atomics).  Then a leg of B with the per-kernel clocks on: the "inlets" clock (one event pair around every launch of k_inlet_values).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = (0.0, 0.0, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1e-4)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda:0")
    n = args.n

    def solver(inlets):
        c = bench.c3_case(prod, n, args.dt, 1)
        c.u_bc[5] = prod.FY_BC_U_ZERO_GRADIENT
        c.p_bc[5], c.p_value[5] = prod.FY_BC_P_FIXED_VALUE, 0.0
        for a in range(3):
            c.u_value[4][a] = V[a]
        if inlets:
            c._inlets = prod.inlets_desc([dict(patch=4, terms=[dict(f=dict(kind="table", points=[(0.0, 1.0), (1e9, 1.0)]), shape=np.tile(V, (n * n, 1)))])])
            c.inlets = c._inlets
        s = prod.Solver(c)
        s.set_particles_device(bench.c3_particles(torch, args.particles, n, 3, dev))
        return s

    a, b = solver(False), solver(True)

    def leg(s, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    leg(a, args.warmup); leg(b, args.warmup)
    uniform, inlet = [], []
    for _ in range(args.rounds):
        uniform.append(leg(a, args.steps))
        inlet.append(leg(b, args.steps))
    # the two flows against each other, and against what two runs of the SAME case differ by (the cloud's scatter adds in the order the atomics arrive)
    dist = lambda x, y: float(np.abs(x.get("U") - y.get("U")).max() / np.abs(x.get("U")).max())
    a2 = solver(False)
    leg(a2, args.warmup + args.rounds * args.steps)
    d_ab, d_aa = dist(a, b), dist(a, a2)
    a2.close()
    b.enable_kernel_timing(True)
    leg(b, args.steps)
    ms, launches = b.kernel_timing("inlets")
    b.enable_kernel_timing(False)
    out = {"cells": n ** 3, "inlet_faces": n * n, "particles": args.particles, "clock": {"inlets": {"ms_per_launch": ms / max(launches, 1), "launches_timed": launches}},
           "step_ms_uniform": uniform, "step_ms_inlet": inlet, "step_ms_difference": sum(inlet) / len(inlet) - sum(uniform) / len(uniform), "U_distance_inlet_vs_uniform": d_ab, "U_distance_uniform_vs_uniform": d_aa}
    print(json.dumps(out))
    a.close(); b.close()


if __name__ == "__main__":
    main()
