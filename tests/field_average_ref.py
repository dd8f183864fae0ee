"""numpy restatement of the fieldAverage arithmetic (include/foamyade_hip.h, fy_average_desc), operation for operation as k_field_average performs it --
every line below is the same IEEE double operation, in the same order and bracketing, with no fused multiply-add -- plus the closed forms the recurrence
amounts to.  The arithmetic is OpenFOAM-6's fieldAverage as recalled (fieldAverageTemplates.C); OpenFOAM is not at hand, so nothing here is pinned to it."""
import numpy as np

SYMM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # symmTensor order xx xy xz yy yz zz


class Item:
    """one averaged field: x is (n,) for a scalar, (n, 3) for a vector; P (with prime2) is (n,) or (n, 6)"""

    def __init__(self, shape, prime2=False, base="time", m=None, P=None, N=0, T=0.0):
        self.vector = len(shape) == 2
        self.prime2, self.base = prime2, base
        self.m = np.zeros(shape) if m is None else np.array(m, dtype=np.float64).reshape(shape)
        pshape = (shape[0], 6) if self.vector else shape
        self.P = None if not prime2 else (np.zeros(pshape) if P is None else np.array(P, dtype=np.float64).reshape(pshape))
        self.N, self.T = int(N), float(T)

    def add(self, x, dt):
        x = np.asarray(x, dtype=np.float64).reshape(self.m.shape)
        dt = float(dt)
        if self.base == "time":
            Dt = self.T + dt
            a, b = (Dt - dt) / Dt, dt / Dt
        else:
            Dt = float(self.N + 1)
            a, b = (Dt - 1.0) / Dt, 1.0 / Dt
        m = self.m
        if self.prime2 and not self.vector:
            P = self.P + m * m
            mn = a * m + b * x
            self.P = (a * P + b * (x * x)) - mn * mn
        elif self.prime2:
            P = self.P.copy()
            for q, (i, j) in enumerate(SYMM):
                P[:, q] = P[:, q] + m[:, i] * m[:, j]
            mn = a * m + b * x
            for q, (i, j) in enumerate(SYMM):
                P[:, q] = (a * P[:, q] + b * (x[:, i] * x[:, j])) - mn[:, i] * mn[:, j]
            self.P = P
        else:
            mn = a * m + b * x
        self.m = mn
        self.N += 1
        self.T += dt


def closed_form(xs, dts, base="time"):
    """(mean, prime2Mean) of the samples xs (each (n,) or (n, 3)) weighted by dts (base time) or equally (base iteration):
    m = sum w x / sum w, P = sum w x_i x_j / sum w - m_i m_j, summed in the plain order"""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    w = np.asarray(dts, dtype=np.float64) if base == "time" else np.ones(len(xs))
    W = w.sum()
    m = sum(wi * x for wi, x in zip(w, xs)) / W
    if xs[0].ndim == 1:
        P = sum(wi * x * x for wi, x in zip(w, xs)) / W - m * m
    else:
        P = np.stack([sum(wi * x[:, i] * x[:, j] for wi, x in zip(w, xs)) / W - m[:, i] * m[:, j] for i, j in SYMM], axis=1)
    return m, P


def in_window(elapsed, dt, start_after=0.0, stop_after=0.0):
    """whether the step that ended at `elapsed` (seconds since the solver was created) is sampled"""
    return elapsed >= start_after - 0.5 * dt and (stop_after <= 0 or elapsed <= stop_after + 0.5 * dt)
