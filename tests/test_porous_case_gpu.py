"""constant/couplingProperties porousZones on the device: a case opened through the reader (fy_foam_case_make_solver / fy_foam_case_make_ldu_solver) steps with the
bits of the hand-built solver given cells_in_box of the same box, and foamYadeHip prints the zone line.  The reader itself: tests/test_porous_case.py."""
import os
import subprocess

import numpy as np
import pytest

from test_porous_case import case_copy, open_case, write

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LO, HI, D, F = (-0.03, -0.03, 0.02), (0.03, 0.03, 0.05), (2e5, 3e5, 4e6), (10.0, 20.0, 250.0)
ENTRY = "porousZones { plate { type DarcyForchheimer; box (-0.03 -0.03 0.02) (0.03 0.03 0.05); d (2e5 3e5 4e6); f (10 20 250); } }\n"


@pytest.fixture
def prod():
    from conftest import load_product
    return load_product()


@pytest.mark.parametrize("kind", ["block", "general"])
def test_a_case_with_a_zone_steps_like_the_hand_built_solver(prod, tmp_path, kind):
    dst = case_copy(tmp_path, kind)
    write(dst, ENTRY)
    fc = open_case(prod, dst, kind)
    U0, p0 = fc.initial_fields()
    if kind == "block":
        s, h = prod.Solver.from_foam_case(fc), prod.Solver(fc.case)
        n, dx = (12, 12, 24), 0.005
        x = [o + (np.arange(m) + 0.5) * dx for o, m in zip((-0.03, -0.03, 0.0), n)]
        K, J, I = np.meshgrid(x[2], x[1], x[0], indexing="ij")
        C = np.stack([I.ravel(), J.ravel(), K.ravel()], axis=1)
        assert np.array_equal(s.get("U").reshape(-1, 3), U0) and np.array_equal(s.get("p"), p0)      # from_foam_case starts from the start time's fields
        h.set("U", U0); h.set("p", p0)
    else:
        s = prod.LduSolver.from_foam_case(fc)
        os.remove(dst / "constant/couplingProperties")
        fc3 = open_case(prod, dst, kind)                                   # the same case without the file: from_foam_case applies no zone
        h = prod.LduSolver.from_foam_case(fc3)
        with pytest.raises(prod.FoamYadeError):
            h.get("porousZone")
        C = h.get("C").reshape(-1, 3)
    cells = prod.cells_in_box(C, LO, HI)
    assert cells.size == (144 * 6 if kind == "block" else 32)
    with pytest.raises(prod.FoamYadeError):
        h.porous_stats()                                                    # the descriptors carry no zones: a solver created from them alone has none
    h.set_porous_zones([dict(name="plate", cells=cells, d=D, f=F)])
    assert np.array_equal(s.get("porousZone"), h.get("porousZone")) and np.count_nonzero(s.get("porousZone")) == cells.size
    for _ in range(3):
        s.step(); h.step()
    for nm in ("U", "p", "mom_bd"):
        assert np.array_equal(s.get(nm), h.get(nm)), nm
    st = s.porous_stats()
    assert len(st) == 1 and st[0]["cells"] == cells.size and st[0]["force"][2] > 0 and np.array_equal(st[0]["force"], h.porous_stats()[0]["force"])
    bd = s.get("mom_bd").reshape(-1, 3)
    assert np.all(bd[cells] > 0)
    s.close(); h.close(); fc.close()


@pytest.mark.parametrize("kind", ["block", "general"])
def test_foamYadeHip_prints_the_zone_line(prod, tmp_path, kind):
    exe = os.path.join(os.path.dirname(HERE), "yade-openfoam-coupling_amd", "bin", "foamYadeHip")
    if not os.path.exists(exe):
        pytest.fail("foamYadeHip has not been built: run __graft_entry__.build()")
    dst = case_copy(tmp_path, kind)
    write(dst, ENTRY)
    out = subprocess.run([exe, "-solver", "pimple", "-case", str(dst)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    want = "Porous zone plate: DarcyForchheimer, %d cells, d (200000 300000 4e+06), f (10 20 250)\n" % (144 * 6 if kind == "block" else 32)
    assert want in out.stdout, out.stdout[:3000]
    assert out.stdout.count("\nTime = ") == 10 and (dst / "0.002").is_dir()
    assert not any("porous" in f.name.lower() for f in (dst / "0.002").rglob("*"))       # nothing of the zones is written to a time directory
