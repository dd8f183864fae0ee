"""The Gaussian particle half on the cell centres of POLYHEDRAL meshes: prisms, regular tetrahedra (distances to centres tie exactly), 2:1 refined polyhedra (cell
volumes 4 : 1) and wavy hexahedra.  tests/test_graded_mesh.py holds the explicit k-d walk to the reference's golden vectors on graded hexahedral blocks; here
product.GeneralMesh(C, V, lo, hi) + FoamYade run against the oracle (oracle.Mesh(..., centres=C, volumes=V) / oracle.particle_action) with C and V from the
restatement's geometry of the meshes of tests/find_cell_ref.py.  4 000 records: mesh vertices, face centres and cell centres (the tie-makers), uniform points, 200
outside.  Tree pre-order, chain, k, ids, found bit for bit; weights, forces and the four fields at gu.RTOL_GPU, as test_particle_parity.py::test_against_oracle_seeded
asserts them.  interpRange follows V[0] (quirk Q7): the radii are a fraction of cbrt(V[0]), and the oracle is asked that at least 90 % of the chains stay <= 12."""
import numpy as np
import pytest

import find_cell_ref as fr
import golden_util as gu
from test_particle_parity import assert_close, seeded_mutable

NAMES = ["prisms_wavy", "tets", "refined_wavy", "hex8_wavy"]
_INPUTS = {}


def inputs(oracle, name):
    """(C, V, lo, hi, fields, records, the oracle's mesh, its result, its fields after the call), formed once"""
    if name in _INPUTS:
        return _INPUTS[name]
    mesh = fr.MESHES[name][0]()
    o = oracle.LduSolver(mesh, 1e-3, 0.01, [0] * 6, [(0, 0, 0)] * 6, [0] * 6)
    C, V = np.array(o.geometry("C")).reshape(-1, 3), np.array(o.geometry("V")).reshape(-1)
    o.close()
    P = np.asarray(mesh["points"], np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    Nc = C.shape[0]
    rs = np.random.RandomState(31)
    x, y, z = C[:, 0], C[:, 1], C[:, 2]
    fields = dict(U=np.stack([0.3 + 1.5 * y - 0.7 * x * z, -0.2 + 0.9 * z * x, 0.1 * x - 0.4 * y * z], axis=1),
                  gradP=np.stack([-50.0 + 300.0 * x, 2000.0 * y * z, -9810.0 + 100.0 * z], axis=1),
                  divT=np.stack([10.0 * y, -5.0 * x, 3.0 * z * x + 0.25], axis=1), ddtU=np.stack([1.0 + x, 2.0 * y, -z], axis=1),
                  vGrad=rs.standard_normal((Nc, 9)))
    fields = {k: np.ascontiguousarray(v) for k, v in fields.items()}
    faces = fr.faces_of(mesh)
    fc = np.array([P[q].mean(axis=0) for q in faces])
    pick = lambda A, n: A[rs.choice(A.shape[0], min(n, A.shape[0]), replace=False)]
    groups = [pick(P, 600), pick(fc, 600), pick(C, 400)]
    h0 = float(np.cbrt(V[0]))
    out = lo + rs.random_sample((200, 3)) * (hi - lo)                       # half 0.3 .. 4 cbrt(V[0]) beyond a side (found in Gaussian mode, quirk Q8), half 6 .. 9
    axis, side = rs.randint(0, 3, 200), rs.randint(0, 2, 200)
    dist = np.where(np.arange(200) % 2 == 0, 0.3 + 3.7 * rs.random_sample(200), 6.0 + 3.0 * rs.random_sample(200)) * h0
    for q in range(200):
        out[q, axis[q]] = lo[axis[q]] - dist[q] if side[q] == 0 else hi[axis[q]] + dist[q]
    groups.append(out)
    groups.append(lo + (0.02 + 0.96 * rs.random_sample((4000 - sum(g.shape[0] for g in groups), 3))) * (hi - lo))
    rec = np.zeros((4000, 10))
    rec[:, 0:3] = np.concatenate(groups)[rs.permutation(4000)]
    rec[:, 3:6] = (rs.random_sample((4000, 3)) * 2.0 - 1.0) * 0.5
    rec[:, 6:9] = (rs.random_sample((4000, 3)) * 2.0 - 1.0) * 0.1
    rec[:, 9] = RADIUS * h0 * (0.6 + 0.8 * rs.random_sample(4000))
    om = oracle.Mesh(Nc, 1, 1, h0, tuple(lo), centres=C, volumes=V, bbmin=lo, bbmax=hi)
    omut = oracle.fresh_mutable(Nc)
    ref = oracle.particle_action(om, fields, omut, rec, np.array([0, 4000], np.int32), 1, RHO_P, RHO_F, NU, threads=8)
    _INPUTS[name] = (C, V, lo, hi, fields, rec, om, ref, omut)
    return _INPUTS[name]


RADIUS, RHO_P, RHO_F, NU, DT = 0.1, 2500.0, 1000.0, 1e-6, 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gaussian_mode_on_polyhedral_cell_centres_matches_the_oracle(product, oracle, name):
    C, V, lo, hi, fields, rec, om, ref, omut = inputs(oracle, name)
    Nc = C.shape[0]
    # ---- what the oracle says of the inputs
    assert (ref["chain_len"] <= 12).mean() >= 0.9, (ref["chain_len"] <= 12).mean()
    assert (ref["found"] == 1).sum() >= 3800 and (ref["found"] == -1).sum() >= 50 and ref["k"].max() > 1
    if name == "refined_wavy":
        assert V.max() / V.min() > 2                      # alpha uses each cell's own volume
    if name == "tets":                                    # regular: a vertex is equally far from the centres of the cells round it, to the last bit for some
        d = np.sort(((C[None, :, :] - rec[:, None, 0:3]) ** 2).sum(axis=2), axis=1)
        assert (d[:, 0] == d[:, 1]).sum() >= 100             # (the 125 vertices and the face centres are all among the records)
    # ---- the device
    mut = seeded_mutable(Nc)
    fy = product.FoamYade(product.GeneralMesh(C, V, lo, hi), fields["U"], fields["gradP"], fields["vGrad"], fields["divT"], fields["ddtU"], (0.0, 0.0, -9.81),
                          mut["uSourceDrag"], mut["alpha"], mut["uSource"], mut["uParticle"], True)
    fy.setScalarProperties(RHO_P, RHO_F, NU)
    assert np.array_equal(fy.tree_preorder(), om.pre)
    fy.setParticles([rec])
    fy.setParticleAction(DT)
    k, ids, w, chain = fy.stencils(0)
    assert np.array_equal(chain, ref["chain_len"])
    assert np.array_equal(k, ref["k"])
    assert np.array_equal(ids, ref["ids"])
    assert np.array_equal(fy.found(0), ref["found"])
    assert_close(w, ref["w"], gu.RTOL_GPU, "weights")
    assert_close(fy.forces(0), ref["force"], gu.RTOL_GPU, "force")
    for nm in ("alpha", "uSource", "uSourceDrag", "uParticle"):
        assert_close(mut[nm], omut[nm], gu.RTOL_GPU, nm)
    fy.close()
