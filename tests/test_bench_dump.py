"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files so that two builds can be compared output for
output.  The sample rule and the size bound on CPU; on the GPU, a small bench run against the same steps driven through the Solver directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT


def test_dump_rows_is_a_fixed_sample():
    assert np.array_equal(bench.dump_rows(1000, 1000), np.arange(1000))
    a, b = bench.dump_rows(10_000_000, 4096), bench.dump_rows(10_000_000, 4096)
    assert np.array_equal(a, b)
    assert a.size == 4096 and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10_000_000


def test_dump_outputs_dtypes_and_sample(tmp_path):
    rng = np.random.default_rng(1)
    forces, found = rng.standard_normal((5000, 6)), np.where(rng.random(5000) < 0.5, 1, -1).astype(np.int32)
    p = rng.standard_normal(300)
    kept = bench.dump_outputs(str(tmp_path), {"forces": forces, "found": found, "p": p}, cap=1000, prefix="rank1_")
    assert kept == {"forces": [1000, 5000], "found": [1000, 5000], "p": [300, 300]}
    rows = bench.dump_rows(5000, 1000)
    f = np.load(tmp_path / "rank1_forces.npy")
    assert f.dtype == np.float64 and np.array_equal(f, forces[rows])
    g = np.load(tmp_path / "rank1_found.npy")
    assert g.dtype == np.float32 and np.array_equal(g, found[rows].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "rank1_p.npy"), p)


def test_dump_stays_under_64_mb():
    # forces 6 + U 3 + p 1 doubles and the found flags as float32, DUMP_ROWS rows each at most (divided by the ranks)
    assert bench.DUMP_ROWS * (6 * 8 + 3 * 8 + 8 + 4) <= 64 * 10 ** 6


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_timed_step(product, tmp_path):
    n, n_part, warmup, steps = 32, 60000, 2, 3
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--n", str(n),
                          "--particles", str(n_part), "--no-cpu-baseline", "--wire", "0", "--no-extras", "--pmc", "0", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout[-2000:]
    j = json.loads(line[0])
    assert j["steps"] == steps and j["ms_per_step"] > 0
    assert j["dumped_outputs"]["rows"] == {"forces": [n_part, n_part], "found": [n_part, n_part], "U": [n ** 3, n ** 3], "p": [n ** 3, n ** 3]}

    # the same warm-up + timed steps driven directly: the dump holds the state after exactly warmup + steps coupled steps
    import torch
    dev = torch.device("cuda", 0)
    s = product.Solver(bench.c3_case(product, n, 1e-4, 1), device=0)
    try:
        rec = bench.c3_particles(torch, n_part, n, 3, dev)
        s.set_particles_device(rec)
        for _ in range(warmup + steps):
            s.step()
        want = {"forces": s.forces(), "found": s.found().astype(np.float32), "U": s.get("U").reshape(-1, 3), "p": s.get("p")}
    finally:
        s.close()
    for name, w in want.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == (np.float32 if name == "found" else np.float64) and got.shape == w.shape, name
        if name == "found":
            assert np.array_equal(got, w)
        else:
            # the deposits' atomics sum in a different order from run to run; the linear solvers stop on a residual (as tests/test_bench_size_parity.py)
            assert np.abs(w).max() > 0, name
            np.testing.assert_allclose(got, w, rtol=0, atol=1e-5 * np.abs(w).max(), err_msg=name)
