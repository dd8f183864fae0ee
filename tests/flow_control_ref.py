"""Flow-rate control (fy_flow_control_desc, the role of OpenFOAM's meanVelocityForce) restated in numpy's long double: the two sums, the correction, the state's
bookkeeping, and the closed form of a plane channel on uniform hexahedra.  Test infrastructure; checked on its own in test_flow_control_ref.py."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def direction(ubar):
    """(flowDir, |Ubar|) as the library forms them: the root of the sum of squares, then one division per component"""
    ubar = np.asarray(ubar, np.float64)
    mag = np.sqrt(ubar[0] * ubar[0] + ubar[1] * ubar[1] + ubar[2] * ubar[2])
    return ubar / mag, float(mag)


def sums(U, rAU, V, flow_dir, w=None):
    """(S (flowDir . U_i) w_i V_i, S rAU_i w_i V_i) and the two lists of terms, in long double"""
    U = np.asarray(U, LD).reshape(-1, 3); rAU = np.asarray(rAU, LD); V = np.asarray(V, LD)
    d = np.asarray(flow_dir, LD)
    w = np.ones_like(V) if w is None else np.asarray(w, LD)
    tu = (U @ d) * w * V
    tr = rAU * w * V
    return tu.sum(), tr.sum(), tu, tr


def kappa(terms):
    """S |terms| / |S terms|: how much a sum's rounding is amplified"""
    tot = np.abs(terms.sum())
    return float(np.abs(terms).sum() / tot) if tot > 0 else 1.0         # (a sum of zeros is exact)


def correction(U, rAU, V, ubar_vec, relaxation=1.0, w=None):
    """one correct(U): dict(ubar, rAU_ave, dGradP, U = the corrected field [n][3], kappa = the larger of the two sums'), all long double but kappa"""
    d, mag = direction(ubar_vec)
    su, sr, tu, tr = sums(U, rAU, V, d, w)
    Vt = np.asarray(V, LD).sum()
    ubar, rave = su / Vt, sr / Vt
    dG = LD(relaxation) * (LD(mag) - ubar) / rave
    Un = np.asarray(U, LD).reshape(-1, 3) + np.asarray(d, LD)[None, :] * (np.asarray(rAU, LD) * dG)[:, None]
    return dict(ubar=ubar, rAU_ave=rave, dGradP=dG, U=Un, kappa=max(kappa(tu), kappa(tr)))


def bulk(U, V, flow_dir, w=None):
    """(S (flowDir . U_i) w_i V_i / V, S |flowDir . U_i| w_i V_i / V): the bulk velocity and the scale of its rounding"""
    su, _, tu, _ = sums(U, np.zeros(len(V)), V, flow_dir, w)
    Vt = np.asarray(V, LD).sum()
    return su / Vt, np.abs(tu).sum() / Vt


class State:
    """gradP0 and dGradP through the three events: every momentum assembly moves dGradP into gradP0, every correction ASSIGNS dGradP (OpenFOAM's quirk), the
    reported gradient is their sum.  Plain doubles: these are single IEEE additions, the same ones the device does"""

    def __init__(self, gradient0=0.0):
        self.gradP0, self.dGradP, self.corrections = float(gradient0), 0.0, 0

    def assemble(self):
        self.gradP0 = self.gradP0 + self.dGradP
        self.dGradP = 0.0
        return self.gradP0

    def correct(self, dGradP):
        self.dGradP = float(dGradP)
        self.corrections += 1

    @property
    def gradient(self):
        return self.gradP0 + self.dGradP


def channel_profile(ny, H, nu, G=1.0):
    """the steady discrete Poiseuille profile of ny uniform cells between two no-slip walls H apart under the uniform source G: Gauss linear laplacian, the wall faces'
    gradient (0 - u) / (dy / 2).  A tridiagonal solve in long double"""
    dy = LD(H) / ny
    A = np.zeros((ny, ny), LD)
    for j in range(ny):
        for nb in (j - 1, j + 1):
            if 0 <= nb < ny:
                A[j, j] += 1; A[j, nb] -= 1
            else:
                A[j, j] += 2                                    # the wall: (u_j - 0) / (dy / 2)
    A *= LD(nu) / (dy * dy)
    b = np.full(ny, LD(G))
    # Thomas algorithm
    a, d, c = np.array([A[j, j - 1] if j else 0 for j in range(ny)], LD), np.array([A[j, j] for j in range(ny)], LD), np.array([A[j, j + 1] if j + 1 < ny else 0 for j in range(ny)], LD)
    for j in range(1, ny):
        m = a[j] / d[j - 1]
        d[j] = d[j] - m * c[j - 1]; b[j] = b[j] - m * b[j - 1]
    u = np.zeros(ny, LD)
    u[-1] = b[-1] / d[-1]
    for j in range(ny - 2, -1, -1):
        u[j] = (b[j] - c[j] * u[j + 1]) / d[j]
    return u


def channel_gradient(ny, H, nu, mag_ubar):
    """the controller's fixed point: G = |Ubar| / c, c = the bulk velocity of the profile under G = 1"""
    c = channel_profile(ny, H, nu).mean()
    return LD(mag_ubar) / c


def viscous_steps(H, nu, dt, floor=1e-10):
    """steps until the slowest viscous mode exp(-nu pi^2 t / H^2) has decayed below `floor`, and that decay factor"""
    n = int(np.ceil(-np.log(floor) * H * H / (nu * np.pi ** 2 * dt)))
    return n, float(np.exp(-nu * np.pi ** 2 * n * dt / (H * H)))
