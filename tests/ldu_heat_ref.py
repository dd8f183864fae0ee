"""numpy restatement of the fluid temperature equation on a general polyhedral mesh (fy_ldu_case.thermal), written from the formulas of DESIGN_FV.md "T equation"
(the LDU form) and include/foamyade_hip.h -- not from the kernels: a dense (A, b) from owner / neighbour, the patch table, the geometry arrays fy_ldu_solver exports
(V, Sf, magSf, w, dcNO, kvec: tests/test_ldu_parity.py pins them to the CPU restatement's) and given phi, alpha, alphaf, nut, nut on the boundary, T of the old time,
Sp and Su; solved with numpy.linalg.solve.  The particle side is heat_transfer_ref.pass_a / pass_b and thermal_loop_ref, which take stencils and know no mesh.

    alpha V (T - T_old) / dt + sum_f F_f T_f - T sum_f F_f - sum_f gam_f (dcNO_f (T_N - T) + kvec_f . (grad T_old)_f) = (Su - Sp T) / rho_cp
    F_f = alphaf_f phi_f (outward), T_f linear | upwind, gam_f = alphaf_f (w Deff_O + (1 - w) Deff_N) |Sf|, Deff = D + nut / Prt,
    grad T_old the Gauss-linear gradient (boundary value: the patch's, or the cell's), the explicit part added to the owner and taken from the neighbour;
    fixedValue face: gb = (D + nut_b / Prt) |Sf| dcNO on the diagonal, (gb - F_b) T_b in the source; zeroGradient face: F_b on the diagonal."""
import numpy as np

ZERO_GRADIENT, FIXED_VALUE = 0, 1
LINEAR, UPWIND = 0, 1
GEOMETRY = ("V", "Sf", "magSf", "w", "dcNO", "kvec")


def addressing(mesh):
    """owner [nF], neighbour [nI], patch_of [nF - nI] and orig_face [nF] as the solver numbers them: the mesh's own internal faces, then one face per matched pair of
    cyclic patches (fy_poly_mesh.patch_neighbour; owner = the lower cell, the face = that cell's), then the other patches' faces in patch order"""
    own, nei = np.asarray(mesh["owner"]), np.asarray(mesh["neighbour"])
    ps, pz = np.asarray(mesh["patch_start"]), np.asarray(mesh["patch_size"])
    pn = mesh.get("patch_neighbour")
    o, n, orig = list(own[:len(nei)]), list(nei), list(range(len(nei)))
    if pn is not None:
        for a, b in enumerate(pn):
            if b < 0 or b < a:
                continue
            for q in range(pz[a]):
                fA, fB = ps[a] + q, ps[b] + q
                cA, cB = own[fA], own[fB]
                o.append(min(cA, cB)); n.append(max(cA, cB)); orig.append(fA if cA < cB else fB)
    patch_of = []
    for a in range(len(ps)):
        if pn is not None and pn[a] >= 0:
            continue
        for q in range(pz[a]):
            o.append(own[ps[a] + q]); orig.append(ps[a] + q); patch_of.append(a)
    return dict(own=np.asarray(o, int), nei=np.asarray(n, int), patch_of=np.asarray(patch_of, int), orig_face=np.asarray(orig, int), n_cells=int(mesh["n_cells"]))


def geometry_of(solver):
    """the arrays of GEOMETRY from anything with a geometry(name) method"""
    g = {nm: np.asarray(solver.geometry(nm), float) for nm in GEOMETRY}
    g["Sf"] = g["Sf"].reshape(-1, 3); g["kvec"] = g["kvec"].reshape(-1, 3)
    return g


def face_alpha(ad, geo, alpha):
    """alphaf: the linear interpolate on an internal face, 1 on the boundary"""
    ni = ad["nei"].size
    af = np.ones(ad["own"].size)
    af[:ni] = geo["w"] * alpha[ad["own"][:ni]] + (1.0 - geo["w"]) * alpha[ad["nei"]]
    return af


def gauss_gradient(ad, geo, T, bc, val):
    ni, nc = ad["nei"].size, ad["n_cells"]
    o, n, bo, pa = ad["own"][:ni], ad["nei"], ad["own"][ni:], ad["patch_of"]
    Sf, w = geo["Sf"], geo["w"]
    Tf = w * T[o] + (1.0 - w) * T[n]
    Tb = np.where(np.asarray(bc)[pa] == FIXED_VALUE, np.asarray(val, float)[pa], T[bo])
    g = np.zeros((nc, 3))
    np.add.at(g, o, Sf[:ni] * Tf[:, None]); np.add.at(g, n, -Sf[:ni] * Tf[:, None]); np.add.at(g, bo, Sf[ni:] * Tb[:, None])
    return g / geo["V"][:, None]


def assemble_T(ad, geo, dt, phi, Told, D, Prt, bc, val, scheme, alpha=None, alphaf=None, nut=None, nut_b=None, Sp=None, Su=None, rho_cp=1.0):
    """(A, b, corr): the dense system and the explicit non-orthogonal flux per internal face.  ad = addressing(mesh), geo = geometry_of(solver); phi [nF] outward of
    the owner; alpha, nut [nc] (None: 1 and 0); alphaf [nF] (None: face_alpha(alpha)); nut_b [nF - nI] (None: the owner's nut); bc, val per patch"""
    ni, nc = ad["nei"].size, ad["n_cells"]
    o, n, bo, pa = ad["own"][:ni], ad["nei"], ad["own"][ni:], ad["patch_of"]
    w, mag, dc, V = geo["w"], geo["magSf"], geo["dcNO"], geo["V"]
    phi, Told = np.asarray(phi, float), np.asarray(Told, float)
    alpha = np.ones(nc) if alpha is None else np.asarray(alpha, float)
    nut = np.zeros(nc) if nut is None else np.asarray(nut, float)
    af = face_alpha(ad, geo, alpha) if alphaf is None else np.asarray(alphaf, float)
    nb = nut[bo] if nut_b is None else np.asarray(nut_b, float)
    bc, val = np.asarray(bc), np.asarray(val, float)
    Deff = D + nut / Prt
    F = af * phi
    Fi, Fb = F[:ni], F[ni:]
    gam = af[:ni] * (w * Deff[o] + (1.0 - w) * Deff[n]) * mag[:ni]
    grad = gauss_gradient(ad, geo, Told, bc, val)
    corr = gam * np.einsum("fk,fk->f", geo["kvec"], w[:, None] * grad[o] + (1.0 - w)[:, None] * grad[n])
    wc = np.where(Fi >= 0, 1.0, 0.0) if scheme == UPWIND else w
    A, b = np.zeros((nc, nc)), np.zeros(nc)
    cells = np.arange(nc)
    A[cells, cells] = alpha * V / dt
    b += alpha * V / dt * Told
    np.add.at(A, (o, o), wc * Fi + gam * dc[:ni]); np.add.at(A, (o, n), (1.0 - wc) * Fi - gam * dc[:ni])
    np.add.at(A, (n, n), -(1.0 - wc) * Fi + gam * dc[:ni]); np.add.at(A, (n, o), -wc * Fi - gam * dc[:ni])
    np.add.at(b, o, corr); np.add.at(b, n, -corr)
    sumF = np.zeros(nc)
    np.add.at(sumF, o, Fi); np.add.at(sumF, n, -Fi); np.add.at(sumF, bo, Fb)
    fixed = bc[pa] == FIXED_VALUE
    gb = (D + nb / Prt) * mag[ni:] * dc[ni:]
    np.add.at(A, (bo, bo), np.where(fixed, gb, Fb))
    np.add.at(b, bo, np.where(fixed, (gb - Fb) * val[pa], 0.0))
    A[cells, cells] -= sumF
    if Sp is not None:
        A[cells, cells] += np.asarray(Sp) / rho_cp
        b += np.asarray(Su) / rho_cp
    return A, b, corr


def solve_T(*args, **kw):
    A, b, _ = assemble_T(*args, **kw)
    return np.linalg.solve(A, b)


# ---- a lattice written as a polyhedral mesh (poly_meshes.hex_block, lattice numbering) against the block's arrays (heat_transfer_ref's layouts)
def lattice_phi(mesh, ad, phi_xyz):
    """phi [nF] of the mesh (outward of the owner) from the block's (phi_x, phi_y, phi_z), oriented along +axis"""
    nx, ny, nz = mesh["shape"]
    ni = ad["nei"].size
    out = np.zeros(ad["own"].size)
    strides = (1, nx, nx * ny)
    for f in range(ni):
        c, d = ad["own"][f], strides.index(ad["nei"][f] - ad["own"][f])
        i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
        out[f] = phi_xyz[d][(i + 1 + (nx + 1) * (j + ny * k), i + nx * (j + 1 + (ny + 1) * k), i + nx * (j + ny * (k + 1)))[d]]
    for q, side in enumerate(ad["patch_of"]):               # (one patch per side, in SIDES order)
        c, d, hi = ad["own"][ni + q], side // 2, side % 2
        i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
        ijk = [i, j, k]; ijk[d] += hi
        i, j, k = ijk
        out[ni + q] = (1.0 if hi else -1.0) * phi_xyz[d][(i + (nx + 1) * (j + ny * k), i + nx * (j + (ny + 1) * k), i + nx * (j + ny * k))[d]]
    return out


def graded_map(shape, h):
    """poly_meshes vertex map that puts the lattice points of a unit box at the faces of cells of sizes h = [hx, hy, hz]"""
    xf = [np.concatenate([[0.0], np.cumsum(a)]) for a in h]

    def m(P):
        Q = P.copy()
        for a in range(3):
            Q[:, a] = xf[a][np.rint(P[:, a] * shape[a]).astype(int)]
        return Q
    return m
