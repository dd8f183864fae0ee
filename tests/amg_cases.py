"""The cases of tests/test_amg_reference.py (CPU) and tests/test_amg_parity.py (HIP): meshes of tests/poly_meshes.py chosen for the branches of
csrc/ldu_amg.hip they reach, with the hierarchy each must give -- [(cells, slots)] per level, from the reference's agglomeration with the face areas
as weights -- and a synthetic level-0 matrix for the tests that run without a solver."""
import numpy as np

import poly_meshes as pm

IN_OUT = [("inlet", [0]), ("outlet", [1]), ("walls", [2, 3]), ("sides", [4, 5])]


class Case:
    def __init__(self, name, mesh, levels, why, passes=3, ref=0, fixed_patch=None):
        """mesh: a callable; ref: the pressure reference cell (unused with fixed_patch: a fixed-value pressure patch, ref_cell = -1 in the solver);
        levels: the expected hierarchy"""
        self.name, self._mesh, self.levels, self.why, self.passes, self.fixed_patch = name, mesh, levels, why, passes, fixed_patch
        self.ref = None if fixed_patch is not None else ref
        self._built = None

    @property
    def mesh(self):
        if self._built is None:
            self._built = self._mesh()
        return self._built

    # the flow that gives the solver its pressure matrix: a lid-driven cavity, or inlet -> outlet with the outlet's pressure fixed
    def solver_args(self):
        npatch = len(self.mesh["patch_start"])
        if self.fixed_patch is not None:
            return dict(u_bc=[0, 1, 0, 1], u_val=[(0.5, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0)], p_bc=[0, 1, 0, 0], p_val=[0, 0.0, 0, 0])
        lidp = 3 if npatch > 3 else 0
        # a cyclic patch keeps its (unused) entry; the lid is ymax where there is one
        u_val = [(0.0, 0.0, 0.0)] * npatch
        pn = self.mesh.get("patch_neighbour")
        if pn is None or pn[lidp] < 0:
            u_val[lidp] = (1.0, 0.0, 0.0)
        return dict(u_bc=[0] * npatch, u_val=u_val, p_bc=[0] * npatch, p_val=None)


def _cyclic():
    L = (1.0, 0.8, 0.6)
    return pm.make_cyclic(pm.hex_block(10, 8, 6, L, pm.wavy_periodic(0.02, L)), [(0, 1), (4, 5)])


CASES = [
    Case("single_level", lambda: pm.hex_block(4, 4, 4, vertex_map=pm.wavy(0.03)), [(64, 6)],
         "64 cells: level 0 alone in the tail, the cycle is the dense inverse of the solver's own matrix"),
    Case("small_renumbered", lambda: pm.hex_block(5, 4, 6, (1.0, 0.8, 1.2), pm.wavy(0.04, (1.0, 0.8, 1.2)), renumber_seed=4), [(120, 6), (26, 11)],
         "aggregates that are no boxes: scale = (120 / 26)^(-1/3), coarse rows of 3 to 11 entries with real padding; a reference cell off aggregate 0", ref=119),
    Case("small_renumbered_1pass", lambda: pm.hex_block(5, 4, 6, (1.0, 0.8, 1.2), pm.wavy(0.04, (1.0, 0.8, 1.2)), renumber_seed=4), [(120, 6), (54, 13)],
         "one pass: pairs and a few triples, scale near 2^(-1/3)", passes=1),
    Case("odd_block", lambda: pm.hex_block(9, 7, 5, vertex_map=pm.wavy(0.03), renumber_seed=3), [(315, 6), (32, 13)],
         "odd edges, the passes stop at 32 = kAmgCoarsest / 2"),
    Case("odd_block_1pass", lambda: pm.hex_block(9, 7, 5, vertex_map=pm.wavy(0.03), renumber_seed=3), [(315, 6), (150, 10), (70, 13), (32, 13)],
         "four levels in one workgroup: the tail at its full kAmgTailMax with level 0 launched", passes=1, ref=200),
    Case("through_flow", lambda: pm.hex_block(10, 10, 10, vertex_map=pm.wavy(0.03), patches=IN_OUT, renumber_seed=1), [(1000, 6), (102, 19), (23, 13)],
         "a fixed-value pressure patch: no reference cell (ref_cell = -1), no point term on any level", fixed_patch=1),
    Case("sheared", lambda: pm.hex_block(12, 12, 12, vertex_map=pm.shear(0.3, 0.1, 0.2), renumber_seed=21), [(1728, 6), (172, 21), (19, 14)],
         "rows 21 slots wide"),
    Case("sheared_1pass", lambda: pm.hex_block(12, 12, 12, vertex_map=pm.shear(0.3, 0.1, 0.2), renumber_seed=21),
         [(1728, 6), (797, 16), (369, 21), (172, 21), (81, 18), (39, 17)],
         "five levels of <= 1024 cells: kAmgTailMax binds, level 1 (797 cells) runs on the launch-per-sweep kernels although it would fit the tail",
         passes=1, ref=1000),
    Case("two_launched_levels", lambda: pm.hex_block(24, 20, 18, vertex_map=pm.wavy(0.03)), [(8640, 6), (1080, 6), (135, 6), (16, 6)],
         "the smallest block with a coarse level over 1024 cells: the launch-per-sweep kernels on L.diag / L.b of level 1", ref=8639),
    Case("prisms", lambda: pm.prism_block(12, 12, 8, vertex_map=pm.wavy(0.02)), [(2304, 5), (288, 6), (36, 6)], "five-faced cells; level 1 wider than level 0"),
    Case("tetrahedra", lambda: pm.tet_block(7, 7, 6, vertex_map=pm.wavy(0.02)), [(1764, 4), (217, 10), (26, 11)], "four-faced cells", ref=1763),
    Case("refined", lambda: pm.refined_block(8, 8, 6, 3), [(960, 9), (120, 9), (30, 11)], "2:1 refined polyhedra: rows of nine on level 0 beside rows of five"),
    Case("line", lambda: pm.hex_block(200, 1, 1, (20.0, 0.1, 0.1)), [(200, 2), (25, 2)], "a chain: rows of one and two entries"),
    Case("line_1pass", lambda: pm.hex_block(200, 1, 1, (20.0, 0.1, 0.1)), [(200, 2), (100, 2), (50, 2)], "clean pairs: scale = 2^(-1/3) exactly", passes=1),
    Case("cyclic", _cyclic, [(480, 6), (60, 6)], "two cyclic pairs folded into internal faces after the mesh's own: every cell has six neighbours", ref=7),
]
BY_NAME = {c.name: c for c in CASES}


def face_geometry(mesh):
    """(point average, area vector) per face: the fan of triangles about the point average"""
    P, off, fp = mesh["points"], mesh["face_offsets"], mesh["face_points"]
    nf = len(off) - 1
    ctr, S = np.zeros((nf, 3)), np.zeros((nf, 3))
    size = np.diff(off)
    for n in np.unique(size):
        fs = np.nonzero(size == n)[0]
        pts = P[fp[off[fs][:, None] + np.arange(n)[None, :]]]                 # [faces, n, 3]
        c = pts.mean(axis=1)
        ctr[fs] = c
        S[fs] = 0.5 * np.cross(np.roll(pts, -1, axis=1) - pts, c[:, None, :] - pts).sum(axis=1)
    return ctr, S


def face_areas(mesh):
    """|S| of the solver's internal faces (the folded cyclic faces after the mesh's own)"""
    import amg_ref
    _, S = face_geometry(mesh)
    a = np.linalg.norm(S, axis=1)
    ni = len(mesh["neighbour"])
    out = list(a[:ni])
    pn = mesh.get("patch_neighbour")
    if pn is not None:
        for pa, pb in enumerate(pn):
            if pb > pa:
                out += list(a[mesh["patch_start"][pa]:mesh["patch_start"][pa] + mesh["patch_size"][pa]])
    assert len(out) == len(amg_ref.internal_faces(mesh)[0])
    return np.asarray(out)


def synthetic_matrix(case):
    """(areas, p_coef, p_diag, centres) of a Laplacian-like matrix on the case's mesh: coefficient = face area / centre distance, diagonal = the row sums, plus the
    reference cell's diagonal doubled (setReference) or area / distance on the faces of the fixed-value patch"""
    import amg_ref
    mesh = case.mesh
    ctr, S = face_geometry(mesh)
    own_all = np.asarray(mesh["owner"])
    n = int(mesh["n_cells"])
    C = np.zeros((n, 3)); cnt = np.zeros(n)
    ni = len(mesh["neighbour"])
    np.add.at(C, own_all, ctr); np.add.at(cnt, own_all, 1)
    np.add.at(C, np.asarray(mesh["neighbour"]), ctr[:ni]); np.add.at(cnt, np.asarray(mesh["neighbour"]), 1)
    C /= cnt[:, None]
    own, nei = amg_ref.internal_faces(mesh)
    areas = face_areas(mesh)
    dist = np.linalg.norm(C[nei] - C[own], axis=1)
    if len(own) > ni:                            # folded faces: the neighbour is seen through the pair; twice the distance to the face instead
        fa = np.concatenate([np.arange(mesh["patch_start"][a], mesh["patch_start"][a] + mesh["patch_size"][a]) for a, b in enumerate(mesh["patch_neighbour"]) if b > a])
        dist[ni:] = 2 * np.linalg.norm(ctr[fa] - C[own_all[fa]], axis=1)
    coef = areas / dist
    diag = np.zeros(n)
    np.add.at(diag, own, coef); np.add.at(diag, nei, coef)
    if case.fixed_patch is not None:
        s, z = int(mesh["patch_start"][case.fixed_patch]), int(mesh["patch_size"][case.fixed_patch])
        f = np.arange(s, s + z)
        np.add.at(diag, own_all[f], np.linalg.norm(S[f], axis=1) / np.linalg.norm(ctr[f] - C[own_all[f]], axis=1))
    else:
        diag[case.ref] *= 2
    return areas, coef, diag, C


def rel(a, b):
    """the distance of a from the reference b, relative to b's largest entry"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def probe_vectors(H, centres, ref):
    """the right-hand sides the cycle is compared on: random, smooth, the unit vectors of the reference cell (cell 0 without one) and of the last cell
    of the last aggregate, the constant"""
    n = H.levels[0].n
    C = np.asarray(centres)
    unit = lambda c: np.eye(1, n, c).ravel()
    agg = H.levels[0].agg
    last = n - 1 if agg is None else int(np.nonzero(agg == agg.max())[0][-1])
    return {"random": np.random.RandomState(8).standard_normal(n),
            "smooth": np.cos(np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1]) * np.cos(2 * np.pi * C[:, 2]),
            "unit_ref": unit(ref if ref is not None else 0), "unit_last": unit(last), "constant": np.ones(n)}


PCG_CUTS = (1, 2, 5)

# d64 per quantity family: the largest distance, over CASES on their synthetic matrices, between amg_ref in float64 and in longdouble, relative to the
# long-double result's largest entry (tests/test_amg_reference.py re-measures it).  What double arithmetic alone costs, the pivot-free elimination of
# the last level included; the device is held to ten times that
D64 = {"coef": 2.3e-16, "diag": 1.2e-15, "inv": 6.2e-13, "cycle": 7.7e-13, "pcg": 4.7e-13}
BOUND_FACTOR = 10.0


def measure_d64(case):
    """{family: distance} of one case"""
    import amg_ref
    areas, coef, diag, C = synthetic_matrix(case)
    H = amg_ref.Hierarchy(case.mesh, areas, coef, diag, case.ref, case.passes, np.longdouble)
    G = amg_ref.Hierarchy(case.mesh, areas, coef, diag, case.ref, case.passes, np.float64)
    out = {"coef": 0.0, "diag": 0.0}
    for a, b in zip(G.levels[1:], H.levels[1:]):
        out["coef"] = max(out["coef"], rel(a.coef, b.coef)); out["diag"] = max(out["diag"], rel(a.diag, b.diag))
    out["inv"] = rel(G.coarse_inv, H.coarse_inv)
    out["cycle"] = max(rel(G.precondition(r), H.precondition(r)) for r in probe_vectors(H, C, case.ref).values())
    rs = np.random.RandomState(5)
    x0 = 0.1 * rs.standard_normal(H.levels[0].n)
    b = np.asarray(H.apply(rs.standard_normal(H.levels[0].n)), np.float64)
    xs, _ = amg_ref.pcg(H.apply, H.precondition, b, x0, max(PCG_CUTS))
    ys, _ = amg_ref.pcg(G.apply, G.precondition, b, x0, max(PCG_CUTS), np.float64)
    out["pcg"] = max(rel(ys[k - 1], xs[k - 1]) for k in PCG_CUTS)
    return out
