#!/usr/bin/env python
"""Porous zones at the benchmark size: the momentum assembly sweep on its own clock, with a zone over one tenth of the cells against the same sweep with none.

    python tools/porous_bench.py [--n 160] [--steps 20] [--warmup 3] [--rounds 3]

The case is bench.py's C3 box (pimpleFoamYade, n^3 cells) without particles.  Two solvers step the same flow from the same random velocity; B carries one zone over
n / 10 z-planes (Darcy and Forchheimer in every component).  The legs alternate, `rounds` times each; in every leg the "mom_assemble" clock (one event pair around the
launch of k_assemble_momentum, so one sample per outer iteration; the C3 case runs one) is read over `steps` steps.  Then k_porous_force's own clock over `steps` calls of porous_stats().  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=160)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1e-4)
    args = ap.parse_args()
    import numpy as np
    import bench
    from __graft_entry__ import load_product
    prod = load_product()
    n = args.n
    U0 = 0.01 * np.random.RandomState(1).standard_normal((n ** 3, 3))

    def solver(zone):
        s = prod.Solver(bench.c3_case(prod, n, args.dt, 1))
        s.set("U", U0)
        if zone:
            k0 = n // 2
            cells = np.arange(k0 * n * n, (k0 + max(n // 10, 1)) * n * n, dtype=np.int32)
            s.set_porous_zones([dict(name="tenth", cells=cells, d=(1e5, 2e5, 3e5), f=(10.0, 20.0, 30.0))])
        return s

    a, b = solver(False), solver(True)

    def leg(s, steps):
        s.enable_kernel_timing(2)                 # 2: the assembly sweep's clock beside the others
        for _ in range(steps):
            s.step()
        ms, launches = s.kernel_timing("mom_assemble")
        s.enable_kernel_timing(False)
        return ms / max(launches, 1)

    leg(a, args.warmup); leg(b, args.warmup)
    plain, zoned = [], []
    for _ in range(args.rounds):
        plain.append(leg(a, args.steps))
        zoned.append(leg(b, args.steps))
    b.enable_kernel_timing(True)
    for _ in range(args.steps):
        st = b.porous_stats()
    ms, launches = b.kernel_timing("porous_force")
    out = {"cells": n ** 3, "zone_cells": st[0]["cells"], "mom_assemble_ms_no_zone": plain, "mom_assemble_ms_zone": zoned,
           "difference_ms": sum(zoned) / len(zoned) - sum(plain) / len(plain), "porous_force_ms_per_call": ms / max(launches, 1), "porous_force_calls_timed": launches}
    print(json.dumps(out))
    a.close(); b.close()


if __name__ == "__main__":
    main()
