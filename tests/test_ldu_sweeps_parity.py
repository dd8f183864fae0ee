"""The FV sweeps of the general-mesh solver on the GPU -- the kernels of csrc/ldu_kernels.hip and the driver in ldu_solver.cpp (step, step_pimple, corrector,
corrector_pimple, solve_vec3, solve_pressure with the diagonal preconditioner) -- against oracle/ldu_oracle.cpp compiled in long double, field by field and
branch by branch (tests/ldu_sweep_cases.py: the cases, the protocol, the names a case leaves out).  tests/test_ldu_sweeps_reference.py holds the CPU oracle's
double build to the same reference without a GPU.

Every iteration count is frozen, so a step is a fixed chain of operations.  A pimpleFoamYade case runs coupled on the device (a few hundred clustered particles,
hold_sources); the alpha / uSourceDrag / uSourceCoupling it leaves are handed to both oracle builds through step(source, alpha, drag), so the FV halves see the
same bits and the particle half, which has its own tests, stays out of the reference.

Bound.  As in tests/test_fv_sweeps_parity.py: `e_oracle` is the largest distance of the double build from the wide one over the case list, per field group and
step, fed with the device's coupling fields; it must lie in 1e-17 .. 1e-12, and the device gets 50 x max(e_oracle, 2^-52), which can therefore never exceed
5e-11.  A coefficient off by 1e-9 lands orders of magnitude above it (tests/test_ldu_sweeps_reference.py; DESIGN.md, parity section, where the measured
distances stand too)."""
import numpy as np
import pytest

import ldu_sweep_cases as lc

pytestmark = pytest.mark.gpu

NAMES = list(lc.CASES)
_device, _oracle = {}, {}


def device_side(product, name):
    """per step (fields, stats, coupling fields) of the HIP solver, once per case"""
    if name in _device:
        return _device[name]
    c = lc.CASES[name]
    names = lc.compared(c)
    pimple = c["solver"] == 1
    s = lc.product_solver(product, c)
    s.hold_sources(True)
    U0, p0 = lc.initial(c)
    s.set("U", U0); s.set("p", p0)
    out = []
    for step in range(2):
        src = lc.external_source(c, step)
        if pimple:
            s.set_particles(lc.records(c, step))
        s.step(src)
        st = s.stats()
        st = dict(st, cont_sum_local=st["cont_err_sum_local"])               # (the oracle's name)
        if pimple:
            cpl = dict(alpha=s.get("alpha"), uSourceDrag=s.get("uSourceDrag"), uSource=s.get("uSourceCoupling"))
        else:
            cpl = dict(alpha=None, uSourceDrag=None, uSource=src)
        fields = {nm: np.asarray(s.geometry(nm) if nm in lc.GEOMETRY else s.get(nm)).ravel() for nm in names}
        if "kvec" in c["omit"]:
            assert np.abs(s.geometry("kvec")).max() < lc.KVEC_NOISE
        out.append((fields, st, cpl))
    s.close()
    _device[name] = out
    return out


def oracle_side(oracle, product, name):
    """(double build, wide build) fed with the device's coupling fields"""
    if name not in _oracle:
        c = lc.CASES[name]
        cpl = [d[2] for d in device_side(product, name)]
        _oracle[name] = (lc.run_oracle(oracle, c, cpl, wide=False), lc.run_oracle(oracle, c, cpl, wide=True))
    return _oracle[name]


@pytest.fixture(scope="module")
def e_oracle(oracle, product):
    e = lc.Envelope()
    for name in NAMES:
        dbl, wide = oracle_side(oracle, product, name)
        for step in range(2):
            w = e.add(name, step, lc.distances(lc.CASES[name], dbl[step], wide[step]))
            print(f"oracle {name:34s} step {step + 1}  " + "  ".join(f"{g} {w[g][0]:.2e} {w[g][1]}" for g in lc.GROUPS))
    print("\n" + e.report())
    e.check_window()
    return e


@pytest.mark.parametrize("name", NAMES)
def test_device_sweeps_match_the_long_double_oracle(product, oracle, e_oracle, name):
    c = lc.CASES[name]
    dev = device_side(product, name)
    dbl, wide = oracle_side(oracle, product, name)
    failures = []
    for step in range(2):
        fields, st, cpl = dev[step]
        # a coupled case must not quietly run fluid-only (uSourceDrag is a coefficient moved to the diagonal with its sign: the drag makes it negative)
        if c["solver"] == 1:
            assert cpl["alpha"].min() < 0.9 and cpl["uSourceDrag"].min() < 0, (cpl["alpha"].min(), cpl["uSourceDrag"].min())
        for side, s in (("device", st), ("oracle", dbl[step][1]), ("wide oracle", wide[step][1])):
            assert lc.counts_ok(c, s), (side, step, lc.expected_counts(c), s["u_iters_total"], s["p_iters_total"])
        for nm, v in fields.items():
            assert np.isfinite(v).all(), nm
        dist = lc.distances(c, (fields, st), wide[step])
        for g, per_name in dist.items():
            bound = e_oracle.bound(g, step)
            for nm, v in per_name.items():
                print(f"{name} step {step + 1} {g:10s} {nm:14s} {v:.2e}  bound {bound:.2e}{'   <-- ABOVE' if v > bound else ''}")
                if v > bound:
                    failures.append((step + 1, nm, v, bound))
    assert not failures, failures
