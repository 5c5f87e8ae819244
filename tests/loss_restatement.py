"""Robust losses (include/nonlin_hip.h: nlh_loss_*) restated in numpy, step by step in the operation order the header
states: one IEEE operation per step, so that the device kernels reproduce Huber and soft-L1 bit for bit (+ - * / sqrt only;
tests/expr_restatement.py already treats sqrt as exact) and Cauchy within the bound of cauchy_bounds(), built the way
expr_restatement builds its own from the measured error of the device library's log1p.  Test infrastructure, not part of
the product."""
import numpy as np

LINEAR, HUBER, SOFT_L1, CAUCHY = 0, 1, 2, 3
KINDS = {"linear": LINEAR, "huber": HUBER, "soft_l1": SOFT_L1, "cauchy": CAUCHY}
ROBUST = ("huber", "soft_l1", "cauchy")
U = 2.0 ** -52

# Error of the device library's log1p in ulp over [1e-12, 1e6], rounded up to an integer: the ceiling of the maximum that
# tests/test_gpu_loss.py::test_log1p_accuracy measures against numpy.longdouble at 2^18 arguments.  The ceiling of a positive
# figure is at least 1, so 1 is the tightest entry that rule can give; the test asserts that the ceiling of what it measures
# IS this entry, so a library whose log1p is off by more than 1 ulp fails there, and the entry cannot be looser than the
# measurement either.
U_LOG1P = 1


def apply(kind, c, r):
    """(out, g, wgt) of the inner residuals r under a loss of scale c (broadcast against r), by the header's table.  A scale
    that is not finite or not positive gives NaN everywhere (every kind but LINEAR)."""
    r = np.asarray(r, dtype=np.float64)
    out, g, wgt = r.copy(), np.ones(r.shape), np.ones(r.shape)
    if kind == LINEAR:
        return out, g, wgt
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), r.shape)
    bad = ~((c > 0.0) & np.isfinite(c))
    with np.errstate(all="ignore"):
        u = r / c
        a = np.fabs(u)
        if kind == HUBER:
            far = ~(a <= 1.0)                                       # NaN lands here
            v = 2.0 * a
            v = v - 1.0
            s = np.sqrt(v)
            out = np.where(far, c * np.copysign(s, u), r)
            g = np.where(far, 1.0 / s, 1.0)
            wgt = np.where(far, 1.0 / a, 1.0)
        elif kind == SOFT_L1:
            z = u * u
            s = np.sqrt(1.0 + z)
            k = np.sqrt(2.0 / (s + 1.0))
            out = c * (u * k)
            g = 1.0 / (s * k)
            wgt = 1.0 / s
        elif kind == CAUCHY:
            z = u * u
            zero = z == 0.0
            l = np.log1p(z)
            s = np.sqrt(l)
            q = 1.0 + z
            w = 1.0 / q
            out = np.where(zero, r, c * np.copysign(s, u))
            g = np.where(zero, 1.0, (w * a) / s)
            wgt = np.where(zero, 1.0, w)
        else:
            raise KeyError(kind)
    nan = np.float64("nan")
    return np.where(bad, nan, out), np.where(bad, nan, g), np.where(bad, nan, wgt)


def residual(kind, c, r):
    return apply(kind, c, r)[0]


def jacobian(kind, c, r, J):
    """J' (m, n) = g_i * J[i][j], g from the inner residual r (m) at the same point."""
    return apply(kind, c, r)[1][:, None] * np.asarray(J)


def rho(kind, z):
    """The loss itself on z = (r / c)^2, in whatever dtype z has: what sum out^2 = c^2 sum rho is held to."""
    if kind == LINEAR:
        return z
    if kind == HUBER:
        return np.where(z <= 1, z, 2 * np.sqrt(z) - 1)
    if kind == SOFT_L1:
        return 2 * z / (np.sqrt(1 + z) + 1)                         # = 2 (sqrt(1 + z) - 1), without its cancellation at small z
    if kind == CAUCHY:
        return np.log1p(z)
    raise KeyError(kind)


def cauchy_bounds(out, g):
    """First-order bounds of |device - numpy| for Cauchy's out and g, as expr_restatement's Num would carry them: l = log1p(z)
    differs by (U_LOG1P + 1) ulp of l (the device function's error, and 1 ulp for numpy's); the exact sqrt halves that and adds
    a rounding of s; out = c * copysign(s, u) adds a rounding of out; g = (wgt * a) / s, wgt and a carrying no error, takes
    s's relative error and adds a rounding of g."""
    k = 0.5 * (U_LOG1P + 1) + 1.0
    return (k + 1.0) * U * np.abs(out), (k + 1.0) * U * np.abs(g)
