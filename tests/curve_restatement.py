"""The built-in curve models (include/nonlin_hip.h: nlh_curve_*) restated in numpy, term by term in the operation order the
header states: one IEEE operation per step, so that the exp-free kind (the Lorentzian) gives the bits of the device
kernels, and the exp kinds differ only by what numpy's exp and the device library's exp differ by.  Every function works
on arrays of abscissae (a row of the data per element) and on any dtype numpy computes in -- complex x included, which the
complex-step check of tests/test_curve_cpu.py uses.  Test infrastructure, not part of the product."""
import numpy as np

GAUSS, LORENTZ, EXPDECAY = 0, 1, 2
KINDS = {"gauss": GAUSS, "lorentz": LORENTZ, "expdecay": EXPDECAY}
MAX_BASE = 8


def nper(kind):
    return 2 if kind == EXPDECAY else 3


def nparams(kind, K, B):
    """n = P K + B + 1, or -1 for what the library refuses."""
    if kind not in (GAUSS, LORENTZ, EXPDECAY) or K < 1 or B < -1 or B > MAX_BASE:
        return -1
    return nper(kind) * K + B + 1


def terms(kind, K, x, t):
    """The K component values at t, in order."""
    out = []
    for k in range(K):
        if kind == GAUSS:
            a, mu, sg = x[3 * k], x[3 * k + 1], x[3 * k + 2]
            d = (t - mu) / sg
            e = np.exp(-0.5 * (d * d))
            out.append(a * e)
        elif kind == LORENTZ:
            a, mu, w = x[3 * k], x[3 * k + 1], x[3 * k + 2]
            d = (t - mu) / w
            q = 1.0 + d * d
            out.append(a / q)
        else:
            a, kk = x[2 * k], x[2 * k + 1]
            e = np.exp(-(kk * t))
            out.append(a * e)
    return out


def baseline(kind, K, B, x, t):
    """Horner from the top; None without a baseline."""
    if B < 0:
        return None
    c = x[nper(kind) * K:]
    b = np.full(np.shape(t), c[B], dtype=np.result_type(x, t))
    for j in range(B - 1, -1, -1):
        b = b * t + c[j]
    return b


def model(kind, K, B, x, t):
    """Model values: s = 0; s = s + term_k; s = s + b."""
    s = np.zeros(np.shape(t), dtype=np.result_type(x, t))
    for term in terms(kind, K, x, t):
        s = s + term
    b = baseline(kind, K, B, x, t)
    if b is not None:
        s = s + b
    return s


def residual(kind, K, B, x, t, y, w=None):
    r = model(kind, K, B, x, t) - y
    if w is not None:
        r = w * r
    return r


def jacobian(kind, K, B, x, t, w=None):
    """The analytic Jacobian as an (m, n) array (column j: the partial with respect to x[j])."""
    cols = []
    for k in range(K):
        if kind == GAUSS:
            a, mu, sg = x[3 * k], x[3 * k + 1], x[3 * k + 2]
            d = (t - mu) / sg
            e = np.exp(-0.5 * (d * d))
            g = ((a * e) * d) / sg
            cols += [e, g, g * d]
        elif kind == LORENTZ:
            a, mu, wd = x[3 * k], x[3 * k + 1], x[3 * k + 2]
            d = (t - mu) / wd
            q = 1.0 + d * d
            g = ((2.0 * a) * d) / ((wd * q) * q)
            cols += [1.0 / q, g, g * d]
        else:
            a, kk = x[2 * k], x[2 * k + 1]
            e = np.exp(-(kk * t))
            cols += [e, -((a * t) * e)]
    p = np.ones(np.shape(t))
    for j in range(B + 1):
        cols.append(p)
        p = p * t
    if w is not None:
        cols = [w * c for c in cols]
    return np.stack(cols, axis=1)


def abs_sum(kind, K, B, x, t, y):
    """sum_k |term_k| + |b| + |y| per row: the scale of the residual's rounding-error bound."""
    s = np.abs(y).astype(np.float64)
    for term in terms(kind, K, x, t):
        s = s + np.abs(term)
    b = baseline(kind, K, B, x, t)
    if b is not None:
        s = s + np.abs(b)
    return s
