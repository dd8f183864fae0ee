"""numpy / math.fsum restatement of the run-time monitors (volFieldValue / surfaceFieldValue, include/foamyade_hip.h "Run-time monitors").

reduce(op, x, m, w) -> (values, bounds): x [n] or [n, 3] the field in the cells / on the faces, m the cell volumes or face areas, w the weight field.  A vector is
reduced component by component.  The value is math.fsum over the terms the device forms, each with the device's one or two roundings, divided by the fsum of the
denominator's terms:
    sum x_i | average x_i / n | volIntegrate, areaIntegrate x_i m_i | volAverage, areaAverage x_i m_i / S m_i
    weightedVolAverage (w_i m_i) x_i / S (w_i m_i) | weightedAverage w_i x_i / S w_i | min, max
The bound: a term carries one rounding (two where the weight is a product itself) and a sum of n terms in any order n - 1 more, so the numerator is off by at most
(n + 1) u S|term_i|, u = 2^-53; the denominator's own sum by the same relative amount, the division by u.  That is (2 n + 3) u S|term_i| / |den|, stated as
4 n u S|term_i| / |den| (n >= 2); den = 1 for sums and integrals.  min and max carry no rounding: bound 0."""
import math

import numpy as np

U = 2.0 ** -53
VOLUME_OPS = ["sum", "average", "volAverage", "volIntegrate", "weightedVolAverage", "min", "max"]
SURFACE_OPS = ["sum", "average", "areaAverage", "areaIntegrate", "weightedAverage", "min", "max"]


def _one(op, x, m, w):
    n = x.size
    if op == "min":
        return float(x.min()), 0.0
    if op == "max":
        return float(x.max()), 0.0
    if op in ("sum", "average"):
        terms, den = x, (float(n) if op == "average" else 1.0)
    elif op in ("volIntegrate", "areaIntegrate", "volAverage", "areaAverage"):
        terms, den = x * m, (math.fsum(m) if op.endswith("Average") else 1.0)
    elif op == "weightedVolAverage":
        wm = w * m
        terms, den = wm * x, math.fsum(wm)
    elif op == "weightedAverage":
        terms, den = w * x, math.fsum(w)
    else:
        raise ValueError(op)
    return math.fsum(terms) / den, 4.0 * n * U * math.fsum(np.abs(terms)) / abs(den)


def reduce(op, x, m=None, w=None):
    x = np.asarray(x, dtype=np.float64)
    cols = [x] if x.ndim == 1 else [x[:, q] for q in range(x.shape[1])]
    out = [_one(op, np.ascontiguousarray(c), m, w) for c in cols]
    return np.array([v for v, _ in out]), np.array([b for _, b in out])


def labels(op, fields, comps):
    out = []
    for nm, c in zip(fields, comps):
        out += [f"{op}({nm})"] if c == 1 else [f"{op}({nm})_{a}" for a in "xyz"]
    return out
