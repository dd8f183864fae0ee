"""Open boundaries on general meshes (inletOutlet, pressureInletOutletVelocity) restated in numpy: the inflow mask, the boundary value and what ONE boundary face adds
to its owner's row of the momentum matrix, by the code the face takes.  The CPU oracle does not know these conditions; this restatement is held to what it must reduce
to in tests/test_open_boundary_ref.py and the device code is held to it (and to the device's own equivalent conditions) in tests/test_open_boundary.py.

Notation (DESIGN_FV.md "Open boundaries"): n = Sf / |Sf|, gm = nu_eff |Sf| dcNO, phi the face's (alpha-weighted) flux out of the domain, U_P the owner's value.
A face adds  dg  to the scalar diagonal,  bd[3]  to the per-component boundary diagonal and  b[3]  to the source."""
import numpy as np

U_FIXED_VALUE, U_ZERO_GRADIENT, U_SLIP, U_INLET_OUTLET, U_PRESSURE_INLET_OUTLET = 0, 1, 2, 3, 4


def inflow_mask(phi_b, open_face):
    """one byte per boundary face: phi < 0 on the faces of the open patches, 0 elsewhere"""
    return ((np.asarray(phi_b) < 0) & np.asarray(open_face, bool)).astype(np.uint8)


def stats(phi_b, open_face):
    """(number of inflow faces, sum of phi over them, sum of phi over the open outflow faces)"""
    phi_b, open_face = np.asarray(phi_b), np.asarray(open_face, bool)
    m = inflow_mask(phi_b, open_face).astype(bool)
    return int(m.sum()), float(phi_b[m].sum()), float(phi_b[open_face & ~m].sum())


def unit_normal(Sf):
    Sf = np.asarray(Sf, np.float64)
    return Sf / np.sqrt((Sf * Sf).sum(axis=-1, keepdims=True))


def pio_diag(n):
    """snGradTransformDiag of the directionMixed condition with value fraction I - n n: sqrt(1 - n_q^2)"""
    n = np.asarray(n, np.float64)
    return np.sqrt(np.maximum(1.0 - n * n, 0.0))


def pio_value(n, uP):
    """U_b = n (n . U_P) on an inflow face of pressureInletOutletVelocity"""
    n, uP = np.asarray(n, np.float64), np.asarray(uP, np.float64)
    return n * (n * uP).sum(axis=-1, keepdims=True)


def face_code(code, inflow):
    """the code of the condition a face equals: an outflow face of an open patch is zeroGradient, an inflow face of inletOutlet fixedValue"""
    if code < U_INLET_OUTLET:
        return code
    if not inflow:
        return U_ZERO_GRADIENT
    return U_FIXED_VALUE if code == U_INLET_OUTLET else U_PRESSURE_INLET_OUTLET


def boundary_value(code, inflow, n, uP, u_val):
    c = face_code(code, inflow)
    uP, n = np.asarray(uP, np.float64), np.asarray(n, np.float64)
    if c == U_FIXED_VALUE:
        return np.asarray(u_val, np.float64)
    if c == U_SLIP:
        return uP - n * (n @ uP)
    if c == U_PRESSURE_INLET_OUTLET:
        return pio_value(n, uP)
    return uP.copy()


def face_contribution(code, inflow, gm, phi, n, uP, u_val=(0.0, 0.0, 0.0)):
    """(dg, bd[3], b[3]) of one boundary face"""
    c = face_code(code, inflow)
    n, uP = np.asarray(n, np.float64), np.asarray(uP, np.float64)
    bd, b = np.zeros(3), np.zeros(3)
    if c == U_FIXED_VALUE:
        return gm, bd, (gm - phi) * np.asarray(u_val, np.float64)
    if c == U_SLIP:
        an = np.abs(n)
        return phi, gm * an, gm * (an * uP - n * (n @ uP))
    if c == U_PRESSURE_INLET_OUTLET:
        dq = pio_diag(n)
        ub = pio_value(n, uP)
        bd = gm * dq - phi * dq
        b = gm * (dq * uP + (ub - uP)) - phi * (ub - (1.0 - dq) * uP)
        return phi, bd, b
    return phi, bd, b


def pio_rAU_shift(gm, phi, n):
    """what the inflow faces of a pressureInletOutletVelocity patch add to V / rAU of their owner over a zeroGradient face: the component mean of (gm - phi) diag_q"""
    return ((np.asarray(gm) - np.asarray(phi))[:, None] * pio_diag(n)).mean(axis=1)
