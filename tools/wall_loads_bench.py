#!/usr/bin/env python
"""Wall loads at the benchmark size: the sample's time on its own clock beside the monitors' three launches, and the coupled step with the wall loads on against off.

    python tools/wall_loads_bench.py [--n 160] [--particles 10000000] [--steps 30] [--warmup 5] [--rounds 3]

The case is bench.py's C3 (pimpleFoamYade, n^3 closed box, particles at rest in the lower 60 %).  The configuration: one forces object over all six sides, wallShearStress
and yPlus on all six sides, every step.  One solver, the wall loads switched off and on in turn, `rounds` times each, `steps` steps per leg timed on the host around a
device synchronisation.  Then a leg with the per-kernel clocks on: the "wall_loads" clock (one event pair around the face kernel and the fold) and, with the
configuration of tools/monitors_bench.py beside it, the "monitors" clock.  Under tools/kstats.sh the two kernels appear by name (k_wall_loads, k_monitor_finalize).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORCES = [dict(name="box", patches=63, rho=1000.0, cofr=(0.0, 0.0, 0.0))]
LOADS = dict(forces=FORCES, wall_shear_stress=63, y_plus=63)
MONITORS = [dict(name="bed", kind="vol", operation="volAverage", fields=["p", "U", "alpha"]), dict(name="pBottom", kind="surface", patch=1 << 4, operation="areaAverage", fields=["p"]),
            dict(name="flowTop", kind="surface", patch=1 << 5, operation="sum", fields=["phi"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1e-4)
    args = ap.parse_args()
    import torch
    import bench
    from __graft_entry__ import load_product
    prod = load_product()
    dev = torch.device("cuda:0")
    s = prod.Solver(bench.c3_case(prod, args.n, args.dt, 1))
    rec = bench.c3_particles(torch, args.particles, args.n, 3, dev)
    s.set_particles_device(rec)

    def leg(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            s.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    leg(args.warmup)
    off, on = [], []
    for _ in range(args.rounds):
        s.set_wall_loads(None)
        leg(2)
        off.append(leg(args.steps))
        s.set_wall_loads(**LOADS)
        leg(2)
        on.append(leg(args.steps))
    s.set_monitors(MONITORS)
    leg(2)
    s.enable_kernel_timing(True)
    leg(args.steps)
    clocks = {}
    for name in ("wall_loads", "monitors"):
        ms, launches = s.kernel_timing(name)
        clocks[name] = {"ms_per_sample": ms / max(launches, 1), "samples_timed": launches}
    s.enable_kernel_timing(False)
    out = {"cells": args.n ** 3, "boundary_faces": 6 * args.n ** 2, "particles": args.particles, "clock": clocks, "step_ms_off": off, "step_ms_on": on,
           "step_ms_difference": sum(on) / len(on) - sum(off) / len(off), "last_forces_row": s.wall_load_rows(0)[1][-1].tolist()}
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
