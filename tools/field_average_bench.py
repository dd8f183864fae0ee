#!/usr/bin/env python
"""fieldAverage at the benchmark size: the kernel's time on its own clock, and the coupled step with averaging on against off.

    python tools/field_average_bench.py [--n 160] [--particles 10000000] [--steps 30] [--warmup 5] [--rounds 3]

The case is bench.py's C3 (pimpleFoamYade, n^3 closed box, particles at rest in the lower 60 %); the items are U, p and alpha with both moments: 31 doubles
moved per cell and launch (x read, m and P read and written).  One solver, averaging switched off and on in turn, `rounds` times each, `steps` steps per
leg timed on the host around a device synchronisation.  Then one leg with the per-kernel clocks on: the "field_average" clock of
fy_solver_get_kernel_timing (an event pair around the launch).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITEMS = [("U", True), ("p", True), ("alpha", True)]
DOUBLES_PER_CELL = 21 + 5 + 5


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
        s.set_field_average(None)
        leg(2)
        off.append(leg(args.steps))
        s.set_field_average(ITEMS)
        leg(2)
        on.append(leg(args.steps))
    s.enable_kernel_timing(True)
    leg(args.steps)
    ms, launches = s.kernel_timing("field_average")
    s.enable_kernel_timing(False)
    cells = args.n ** 3
    nbytes = 8 * DOUBLES_PER_CELL * cells
    kernel_ms = ms / max(launches, 1)
    out = {"cells": cells, "particles": args.particles, "items": [f"{f}{' + prime2Mean' if p else ''}" for f, p in ITEMS], "bytes_per_launch": nbytes,
           "kernel_ms": kernel_ms, "kernel_launches_timed": launches, "kernel_TB_per_s": nbytes / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else None,
           "step_ms_off": off, "step_ms_on": on, "step_ms_difference": sum(on) / len(on) - sum(off) / len(off), "samples": s.average_state(0)[0]}
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
