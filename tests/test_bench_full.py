"""bench.py without --full prints the headline line alone; --full adds the records beside it (here the CPU baseline with its parity leg, the one
record a small non-default case carries)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "moving", "c2", "general_mesh", "drop_in_path", "roofline_pEqn_laplacian_past_infinity_cache", "exchange_wait")


@pytest.mark.parametrize("extra", [["--pmc", "1"], ["--ref-as-written"]])
def test_an_explicit_request_beside_the_headline_needs_full(extra):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2"] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "add --full" in r.stderr, (r.returncode, r.stderr[-500:])


def bench_line(args):
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_cpu_baseline():
    n, n_part = 32, 60000
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--n", str(n), "--particles", str(n_part)]
    plain = bench_line(args)
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert not [k for k in FULL_ONLY if k in plain], sorted(plain)

    full = bench_line(args + ["--full", "--wire", "0"])
    assert all(k in full for k in HEADLINE) and full["metric"] == plain["metric"] and full["unit"] == plain["unit"]
    cb = full["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["single_thread_value"] > 0
    par = cb["parity_at_bench_size"]
    assert "error" not in par, par
    assert par["particles"] == n_part and par["cells"] == n ** 3
    assert par["k_equal"] and par["ids_equal"] and par["found_equal"], par
    assert par["step1"]["force"] <= 1e-10, par                    # (exact inputs on both sides: tests/test_bench_size_parity.py's particle tolerance)
