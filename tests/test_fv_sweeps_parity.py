"""The FV sweeps of the block solver on the GPU -- the kernels of fv_kernels.hip and the driver in fv_solver.cpp (step, corrector, solve_vec3,
turbulence_correct) -- against oracle/fv_oracle.cpp compiled in long double, field by field and branch by branch (tests/fv_sweep_cases.py: the cases, the
protocol, the names a case leaves out).  tests/test_fv_sweeps_reference.py holds the CPU oracle's double build to the same reference without a GPU.

Every iteration count is frozen, so a step is a fixed chain of operations.  The device runs coupled (a few hundred clustered particles, hold_sources); the
alpha / uSource / uSourceDrag it leaves are written into both oracle builds where setParticleAction stands, so the FV halves see the same bits and the
particle half, which has its own tests, stays out of the reference.

Bound.  As in tests/test_mg_parity.py: `e_oracle` is the largest distance of the double build from the wide one over the case list, per field group (assembled
before any solve / after the predictor / after the pressure solve) and step, fed with the device's coupling fields; it must lie in 1e-17 .. 1e-12, and the
device gets 50 x max(e_oracle, 2^-52) -- contraction, summation order, single-reduction PCG, the Cholesky coarsest level -- which can therefore never exceed
5e-11.  A coefficient off by 1e-9 lands orders of magnitude above it (parity section, where the measured distances stand too)."""
import os

import numpy as np
import pytest

import fv_sweep_cases as fc

pytestmark = pytest.mark.gpu

NAMES = list(fc.CASES)
_device, _oracle = {}, {}


class Switches:
    """kernel switches for the solvers created inside the block (the library reads them when a solver is created); on the way out they are removed and one
    solver is created so that the library reads them again"""

    def __init__(self, product, env):
        self.product, self.env, self.old = product, env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        if self.env:
            self.product.Solver(self.product.make_case(0, 8, 8, 8, 0.1, 1e-3, 0.01, p_solver=1)).close()


def device_side(product, name):
    """per step (fields, stats, coupling fields) of the HIP solver, once per case"""
    if name in _device:
        return _device[name]
    c = fc.CASES[name]
    names = fc.compared(c)
    with Switches(product, c["env"]):
        pc = fc.product_case(product, c)
        s = product.VirtualSlabs(pc, c["slabs"]) if c["slabs"] > 1 else product.Solver(pc)
        solvers = s.solvers if c["slabs"] > 1 else [s]
        for q in solvers:
            q.hold_sources(True)
            if c["force_models"]:
                q.set_force_models(c["force_models"])
        U0, p0 = fc.initial(c)
        s.set("U", U0); s.set("p", p0)
        out = []
        for step in range(2):
            s.set_particles(fc.records(c, step) if c["couple"] else None)
            s.step()
            st = s.stats()[0] if c["slabs"] > 1 else s.stats()
            st = dict(st, cont_sum_local=st["cont_err_sum_local"])               # (the oracle's name)
            cpl = {nm: s.get(nm) for nm in ("alpha", "uSource", "uSourceDrag")}
            out.append(({nm: s.get(nm) for nm in names}, st, cpl))
        s.close()
    _device[name] = out
    return out


def oracle_side(oracle, product, name):
    """(double build, wide build) fed with the device's coupling fields"""
    if name not in _oracle:
        c = fc.CASES[name]
        cpl = [d[2] for d in device_side(product, name)]
        _oracle[name] = (fc.run_oracle(oracle, c, cpl, wide=False), fc.run_oracle(oracle, c, cpl, wide=True))
    return _oracle[name]


@pytest.fixture(scope="module")
def e_oracle(oracle, product):
    e = fc.Envelope()
    for name in NAMES:
        dbl, wide = oracle_side(oracle, product, name)
        for step in range(2):
            w = e.add(name, step, fc.distances(fc.CASES[name], dbl[step], wide[step]))
            print(f"oracle {name:45s} step {step + 1}  " + "  ".join(f"{g} {w[g][0]:.2e} {w[g][1]}" for g in fc.GROUPS))
    print("\n" + e.report())
    e.check_window()
    return e


@pytest.mark.parametrize("name", NAMES)
def test_device_sweeps_match_the_long_double_oracle(product, oracle, e_oracle, name):
    c = fc.CASES[name]
    dev = device_side(product, name)
    dbl, wide = oracle_side(oracle, product, name)
    failures = []
    for step in range(2):
        fields, st, cpl = dev[step]
        # a case must not quietly run fluid-only (uSourceDrag is a coefficient moved to the diagonal with its sign: the drag makes it negative)
        if c["couple"] and c["solver"] == 1:
            assert cpl["alpha"].min() < 0.9 and cpl["uSourceDrag"].min() < 0, (cpl["alpha"].min(), cpl["uSourceDrag"].min())
        elif c["couple"]:
            assert np.abs(cpl["uSource"]).max() > 0
        for side, s in (("device", st), ("oracle", dbl[step][1]), ("wide oracle", wide[step][1])):
            assert fc.counts_ok(c, s), (side, step, fc.expected_counts(c), s["u_iters_total"], s["p_iters_total"])
        for v in fields.values():
            assert np.isfinite(v).all()
        dist = fc.distances(c, (fields, st), wide[step])
        for g, per_name in dist.items():
            bound = e_oracle.bound(g, step)
            for nm, v in per_name.items():
                print(f"{name} step {step + 1} {g:9s} {nm:14s} {v:.2e}  bound {bound:.2e}{'   <-- ABOVE' if v > bound else ''}")
                if v > bound:
                    failures.append((step + 1, nm, v, bound))
    assert not failures, failures


def test_matrix_diagnostics_are_read_only_and_refused_where_the_storage_is_reused(product):
    s = product.Solver(fc.product_case(product, fc.CASES["pimple_box_linear"]))
    for nm in ("mom_an3", "phiHbyA_y"):
        with pytest.raises(product.FoamYadeError, match="read-only"):
            s.set(nm, np.zeros(s._size(nm)))
    s.close()
    s = product.Solver(fc.product_case(product, fc.CASES["pimple_kEpsilon"]))
    with pytest.raises(product.FoamYadeError, match="turbulence transport solve"):
        s.get("mom_an0")
    s.close()


def test_every_switch_reaches_its_path(product):
    """what the driver decides from the switches is visible from outside: the unfused path keeps the stored tensor, the default one refuses it"""
    for env, stored in (({}, False), ({"FOAMYADE_NO_TILED_STRESS": "1"}, True)):
        with Switches(product, env):
            s = product.Solver(fc.product_case(product, fc.CASES["pimple_box_19x11x7"]))
            try:
                s.get("stress_G")
                got = True
            except product.FoamYadeError:
                got = False
            s.close()
        assert got == stored
