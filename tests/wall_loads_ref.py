"""numpy restatement, in np.longdouble, of the wall loads (forces / wallShearStress / yPlus; include/foamyade_hip.h "Wall loads") from what a solver lets one read.

A mesh is a dict of arrays in the solver's face order (internal faces first, then the boundary faces in the order of "p_boundary"):
    owner [nF], neighbour [nI], Sf [nF, 3], magSf [nF], Cf [nF, 3], V [nc], w [nI] (the owner's weight), patch [nb], delta [nb], y [nb], kgeo, F
general_mesh(solver, mesh) reads them from an LduSolver (delta = "dcNO" on the boundary faces, y = "nearWallDist"); block_mesh(nx, ny, nz, dx | grading, origin) forms them
from the block's extents and cell sizes (delta = 2 / h, y = h / 2 of the owner along the face's normal).  F = the most faces a cell has; kgeo = the roundings the
device spends on a geometric quantity the restatement holds (almost) exactly: 0 where the solver's own arrays are read, 3 on the block (an area or volume is a product of
two or three cell sizes, a node coordinate of a graded block a running sum -- see block_mesh).

face_loads(mesh, fields) restates steps 1-6 for EVERY boundary face and returns, per quantity, the value and a majorant: the same expression with every term replaced by
its absolute value and every difference by a sum.  A value formed by K rounded operations from exact inputs is off by at most K u majorant (u = 2^-53) to first order
(the running error bound of a sum of products).  The operation counts along the dependency chains, written out:
    KG   an entry of G_P = (1/V) S Sf (x) U_f: the face value w a + (1 - w) b: 4; times the slot coefficient (itself sg Sf w / V: 3): 1; the sum over F faces and the
         cell's own share: F; geometry: kgeo                                                                                      KG = F + 8 + kgeo
    Ks   s_j = (U_b - U_P) delta: 2, delta on the block 1 more                                                                    Ks = 3
    KR   n_i = Sf_i / |Sf|: 1 + kgeo; (n . G)_j: KG + 1 + 1 + 2; s_j - (n . G)_j: 1; n_i (...): 1; G_ij + ...: 1; twoSymm: 1; the trace / 3: 3; dev: 1;
         nuEff = nu + nut_b: 1; times -nuEff: 1                                                                                    KR = KG + 16 + kgeo
    wallShearStress_j = -(n . R)_j: KR + 1 + 3                                                                                    Kw = KR + 4
    fV_j = rho (Sf . R)_j: KR + 4 + kgeo; fP_j = (rho Sf_j)(p_b - pRef): 3 + kgeo; a moment (Cf - CofR) x f: the force's chain + 1 + kgeo + 2
    yPlus: a product of positive factors, so the bound is relative: Cmu^1/4 y sqrt(k) / nu: 6 + kgeo (Cmu^1/4 and the square root included);
           y sqrt(nuEff |s|) / nu with |s| = sqrt(s . s): Ks + 1 + 2 + 1 + 1 + 1 + 1 + 1 + 1 + kgeo                               Ky = 12 + kgeo
    a sum over N faces in any order: N more; the average's division: 1 more
The restatement's own rounding (2^-64 per operation) is 2^-11 of these bounds and is covered by rounding every count up by one (the "+ 1" in bound()).
min and max carry no rounding of their own: the test holds them bit for bit to the min and max of the device's per-face field."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SIDES = ["x-", "x+", "y-", "y+", "z-", "z+"]


def bound(k, majorant):
    return (k + 1) * U * np.asarray(majorant, dtype=np.float64)


def block_mesh(nx, ny, nz, dx=None, grading=None, origin=(0.0, 0.0, 0.0)):
    """kgeo = 3: a face area h h is one rounding and a volume (h h) h two on the device; a node of a graded block is the running sum the solver forms in double (formed
    here in the same order in double, so that it is the same number) and a centre one or two more roundings"""
    n = (nx, ny, nz)
    h = [np.full(n[a], dx, dtype=np.float64) for a in range(3)] if grading is None else [np.asarray(a, dtype=np.float64) for a in grading]
    if grading is None:
        node = [LD(origin[a]) + np.arange(n[a] + 1).astype(LD) * LD(dx) for a in range(3)]
        mid = [LD(origin[a]) + (np.arange(n[a]).astype(LD) + LD(0.5)) * LD(dx) for a in range(3)]
    else:
        node =[np.array([float(x) for x in _running(origin[a], h[a])], dtype=np.float64).astype(LD) for a in range(3)]
        mid = [LD(0.5) * (node[a][:-1] + node[a][1:]) for a in range(3)]
    hl = [a.astype(LD) for a in h]
    c = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    I, J, K = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")      # [i, j, k]
    ct = c.transpose(2, 1, 0)                                                              # ct[i, j, k]
    V = np.zeros(nx * ny * nz, dtype=LD)
    V[ct.ravel()] = (hl[0][I] * hl[1][J] * hl[2][K]).ravel()
    idx = [I, J, K]

    def area(d, sl):
        a, b = [q for q in range(3) if q != d]
        return (hl[a][idx[a][sl]] * hl[b][idx[b][sl]]).ravel()

    own, nei, Sf, w = [], [], [], []
    for d in range(3):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[d] = slice(0, n[d] - 1); hi[d] = slice(1, n[d])
        lo, hi = tuple(lo), tuple(hi)
        own.append(ct[lo].ravel()); nei.append(ct[hi].ravel())
        A = area(d, lo)
        S = np.zeros((A.size, 3), dtype=LD); S[:, d] = A
        Sf.append(S)
        hlo, hhi = hl[d][idx[d][lo]].ravel(), hl[d][idx[d][hi]].ravel()
        w.append(hhi / (hlo + hhi))
    nI = sum(a.size for a in own)
    bown, bSf, bCf, patch, delta, y = [], [], [], [], [], []
    for side in range(6):
        d, s = side // 2, side % 2
        sl = [slice(None)] * 3
        sl[d] = n[d] - 1 if s else 0
        sl = tuple(sl)
        # the read-outs' order: the lower remaining axis fastest
        cells = ct[sl].T.ravel()
        ii = [np.broadcast_to(idx[a][sl], ct[sl].shape).T.ravel() for a in range(3)]
        a, b = [q for q in range(3) if q != d]
        A = hl[a][ii[a]] * hl[b][ii[b]]
        S = np.zeros((A.size, 3), dtype=LD); S[:, d] = A if s else -A
        X = np.zeros((A.size, 3), dtype=LD)
        for q in range(3):
            X[:, q] = node[q][n[q] if s else 0] if q == d else mid[q][ii[q]]
        bown.append(cells); bSf.append(S); bCf.append(X); patch.append(np.full(A.size, side))
        delta.append(LD(2.0) / hl[d][ii[d]]); y.append(LD(0.5) * hl[d][ii[d]])
    Sf_all = np.concatenate(Sf + bSf)
    Cf = np.concatenate([np.zeros((nI, 3), dtype=LD)] + bCf)
    return dict(owner=np.concatenate(own + bown), neighbour=np.concatenate(nei), Sf=Sf_all, magSf=np.abs(Sf_all).sum(axis=1), Cf=Cf, V=V, w=np.concatenate(w), nI=nI,
                patch=np.concatenate(patch), delta=np.concatenate(delta), y=np.concatenate(y), kgeo=3, F=6, names=SIDES)


def _running(x0, h):
    out = [float(x0)]
    for v in h:
        out.append(out[-1] + float(v))
    return out


def folded_addressing(mesh):
    """(owner, neighbour, patch of each boundary face) in the SOLVER's face order for a mesh with cyclic pairs (mesh["patch_neighbour"]): the mesh's internal faces, then
    one internal face per pair of cyclic faces (pairs a < b, face q of a with face q of b; owner = the lower of the two cells), then the other patches' faces in order"""
    own, nei = np.asarray(mesh["owner"]), np.asarray(mesh["neighbour"])
    ps, pz, pn = np.asarray(mesh["patch_start"]), np.asarray(mesh["patch_size"]), np.asarray(mesh["patch_neighbour"])
    nI = nei.size
    o, n, bo, bp = [own[:nI]], [nei], [], []
    for a in range(len(ps)):
        b = pn[a]
        if b < 0:
            bo.append(own[ps[a]:ps[a] + pz[a]]); bp.append(np.full(pz[a], a))
        elif a < b:
            cA, cB = own[ps[a]:ps[a] + pz[a]], own[ps[b]:ps[b] + pz[b]]
            o.append(np.minimum(cA, cB)); n.append(np.maximum(cA, cB))
    return np.concatenate(o + bo), np.concatenate(n), np.concatenate(bp)


def general_mesh(s, owner, neighbour, patch_size, patch=None):
    """the solver's own geometry arrays.  A mesh without cyclic pairs: the caller's face order is the solver's; with them: owner, neighbour and patch (per boundary
    face) from folded_addressing"""
    magSf = s.get("magSf").astype(LD)
    nF = magSf.size
    nb = s.get("p_boundary").size
    nI = nF - nb
    owner = np.asarray(owner)
    faces_of = np.bincount(owner, minlength=s.get("V").size) + np.bincount(np.asarray(neighbour)[:nI], minlength=s.get("V").size)
    return dict(owner=owner, neighbour=np.asarray(neighbour)[:nI], Sf=s.get("Sf").astype(LD), magSf=magSf, Cf=s.get("Cf").astype(LD), V=s.get("V").astype(LD),
                w=s.get("w").astype(LD)[:nI], nI=nI, patch=np.concatenate([np.full(z, q) for q, z in enumerate(patch_size)]) if patch is None else np.asarray(patch), delta=s.get("dcNO").astype(LD)[nI:],
                y=s.get("nearWallDist").astype(LD), kgeo=0, F=int(faces_of.max()), names=[f"patch{q}" for q in range(len(patch_size))])


def face_loads(m, Uc, Ub, pb, nutb, nu, k=None, wall_fn=None, cmu25=0.0):
    """steps 1-6 on every boundary face.  Uc [nc, 3], Ub [nb, 3], pb [nb], nutb [nb] as read; k [nc] and wall_fn [nb] (bool) where a patch carries nutkWallFunction.
    Returns a dict: n, R, R_mag [nb, 3, 3], wss, wss_mag [nb, 3], yplus [nb], K (the operation counts)"""
    nI, own = m["nI"], m["owner"]
    nb = own.size - nI
    Uc, Ub, pb, nutb = np.asarray(Uc).astype(LD).reshape(-1, 3), np.asarray(Ub).astype(LD).reshape(-1, 3), np.asarray(pb).astype(LD), np.asarray(nutb).astype(LD)
    nc = Uc.shape[0]
    # 1. G_P = (1/V) S Sf (x) U_f, and its majorant
    w = m["w"][:, None]
    Uf = np.concatenate([w * Uc[own[:nI]] + (1 - w) * Uc[m["neighbour"]], Ub])
    Uf_mag = np.concatenate([w * np.abs(Uc[own[:nI]]) + (1 - w) * np.abs(Uc[m["neighbour"]]), np.abs(Ub)])
    G = np.zeros((nc, 3, 3), dtype=LD); Gm = np.zeros((nc, 3, 3), dtype=LD)
    T = m["Sf"][:, :, None] * Uf[:, None, :]
    Tm = np.abs(m["Sf"])[:, :, None] * Uf_mag[:, None, :]
    np.add.at(G, own, T); np.add.at(G, m["neighbour"], -T[:nI])
    np.add.at(Gm, own, Tm); np.add.at(Gm, m["neighbour"], Tm[:nI])
    G /= m["V"][:, None, None]; Gm /= m["V"][:, None, None]
    bo = own[nI:]
    GP, GPm = G[bo], Gm[bo]
    Sf, A = m["Sf"][nI:], m["magSf"][nI:]
    n = Sf / A[:, None]
    an = np.abs(n)
    # 2. s = (U_b - U_P) delta
    s = (Ub - Uc[bo]) * m["delta"][:, None]
    sm = (np.abs(Ub) + np.abs(Uc[bo])) * m["delta"][:, None]
    # 3. G_b = G_P + n (x) (s - n . G_P)
    nG = np.einsum("fi,fij->fj", n, GP); nGm = np.einsum("fi,fij->fj", an, GPm)
    Gb = GP + n[:, :, None] * (s - nG)[:, None, :]
    Gbm = GPm + an[:, :, None] * (sm + nGm)[:, None, :]
    # 4. R_b = -nuEff dev(twoSymm(G_b))
    S2 = Gb + Gb.transpose(0, 2, 1); S2m = Gbm + Gbm.transpose(0, 2, 1)
    tr = np.trace(S2, axis1=1, axis2=2) / 3; trm = np.trace(S2m, axis1=1, axis2=2) / 3
    eye = np.eye(3, dtype=LD)[None]
    nuEff = LD(nu) + nutb
    R = -nuEff[:, None, None] * (S2 - tr[:, None, None] * eye)
    Rm = nuEff[:, None, None] * (S2m + trm[:, None, None] * eye)
    # 5. wallShearStress = -n . R_b
    wss = -np.einsum("fi,fij->fj", n, R); wssm = np.einsum("fi,fij->fj", an, Rm)
    # 6. yPlus
    smag = np.sqrt((s * s).sum(axis=1))
    yp = m["y"] * np.sqrt(nuEff * smag) / LD(nu)
    if wall_fn is not None and np.any(wall_fn):
        kP = np.asarray(k).astype(LD)[bo]
        yp = np.where(wall_fn, LD(cmu25) * m["y"] * np.sqrt(kP) / LD(nu), yp)
    kg = m["kgeo"]
    KG = m["F"] + 8 + kg
    KR = KG + 16 + kg
    return dict(n=n, R=R, R_mag=Rm, wss=wss, wss_mag=wssm, yplus=yp, pb=pb, Sf=Sf, Cf=m["Cf"][nI:], K=dict(G=KG, R=KR, wss=KR + 4, fV=KR + 4 + kg, fP=3 + kg, mom=3 + kg, y=12 + kg))


def forces_row(fl, idx, rho, p_ref, cofr):
    """step 7 over the faces idx: the 12 values Fp, Fv, Mp, Mv and their bounds"""
    rho, p_ref, cofr = LD(rho), LD(p_ref), np.asarray(cofr).astype(LD)
    Sf, R, Rm, K = fl["Sf"][idx], fl["R"][idx], fl["R_mag"][idx], fl["K"]
    N = len(idx)
    fP = rho * Sf * (fl["pb"][idx] - p_ref)[:, None]
    fPm = rho * np.abs(Sf) * (np.abs(fl["pb"][idx]) + abs(p_ref))[:, None]
    fV = rho * np.einsum("fi,fij->fj", Sf, R)
    fVm = rho * np.einsum("fi,fij->fj", np.abs(Sf), Rm)
    r = fl["Cf"][idx] - cofr; rm = np.abs(fl["Cf"][idx]) + np.abs(cofr)

    def crossm(a, b):
        return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)
    vals = [fP, fV, np.cross(r, fP), np.cross(r, fV)]
    mags = [fPm, fVm, crossm(rm, fPm), crossm(rm, fVm)]
    ks = [K["fP"], K["fV"], K["fP"] + K["mom"], K["fV"] + K["mom"]]
    v = np.concatenate([x.sum(axis=0) for x in vals])
    b = np.concatenate([bound(kk + N, x.sum(axis=0).astype(np.float64)) for kk, x in zip(ks, mags)])
    return v.astype(np.float64), b


def wss_bound(fl):
    return bound(fl["K"]["wss"], fl["wss_mag"].astype(np.float64))


def yplus_bound(fl):
    return bound(fl["K"]["y"], fl["yplus"].astype(np.float64))


def yplus_average(fl, idx):
    yp = fl["yplus"][idx]
    return float(yp.sum() / len(idx)), float(bound(fl["K"]["y"] + len(idx) + 1, float(yp.sum()) / len(idx)))


def labels_forces():
    return [f"{g}_{a}" for g in ("Fp", "Fv", "Mp", "Mv") for a in "xyz"]
