#!/usr/bin/env python
"""Run-time monitors at the benchmark size: the sample's time on its own clock, and the coupled step with the monitors on against off.

    python tools/monitors_bench.py [--n 160] [--particles 10000000] [--steps 30] [--warmup 5] [--rounds 3]

The case is bench.py's C3 (pimpleFoamYade, n^3 closed box, particles at rest in the lower 60 %).  The configuration: one volume object over p, U and alpha
(volAverage) and two surface objects (areaAverage(p) on the bottom, sum(phi) on the top).  The cell kernel reads 5 doubles per cell (the uniform block's volume is a
kernel argument).  One solver, the monitors switched off and on in turn, `rounds` times each, `steps` steps per leg timed on the host around a device
synchronisation.  Then two legs with the per-kernel clocks on: the "monitors" clock of fy_solver_get_kernel_timing (one event pair around the sample's launches) with
all three objects -- cells, faces, finalize -- and with the volume object alone -- cells, finalize.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOLUME = dict(name="bed", kind="vol", operation="volAverage", fields=["p", "U", "alpha"])
OBJECTS = [VOLUME, dict(name="pBottom", kind="surface", patch=1 << 4, operation="areaAverage", fields=["p"]),
           dict(name="flowTop", kind="surface", patch=1 << 5, operation="sum", fields=["phi"])]
DOUBLES_PER_CELL = 5


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
        s.set_monitors(None)
        leg(2)
        off.append(leg(args.steps))
        s.set_monitors(OBJECTS)
        leg(2)
        on.append(leg(args.steps))
    clocks = {}
    for label, objs in (("all", OBJECTS), ("volume_only", [VOLUME])):
        s.set_monitors(objs)
        leg(2)
        s.enable_kernel_timing(True)
        leg(args.steps)
        ms, launches = s.kernel_timing("monitors")
        s.enable_kernel_timing(False)
        clocks[label] = {"ms_per_sample": ms / max(launches, 1), "samples_timed": launches}
    rows = s.monitor_rows(0)[1]
    cells = args.n ** 3
    nbytes = 8 * DOUBLES_PER_CELL * cells
    vol_ms = clocks["volume_only"]["ms_per_sample"]
    out = {"cells": cells, "particles": args.particles, "objects": [o["name"] for o in OBJECTS], "cell_kernel_bytes": nbytes, "clock": clocks,
           "volume_only_TB_per_s_lower_bound": nbytes / (vol_ms * 1e-3) / 1e12 if vol_ms > 0 else None,
           "step_ms_off": off, "step_ms_on": on, "step_ms_difference": sum(on) / len(on) - sum(off) / len(off), "last_row": rows[-1].tolist()}
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
