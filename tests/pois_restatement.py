"""Poisson likelihood fits (include/nonlin_hip.h: nlh_pois_*) restated in numpy, step by step in the operation order the
header states: one IEEE operation per step, so that the device kernels reproduce every row that reaches no library function
bit for bit (masked, y = 0, the series, floor rows on those) and the others within the bounds built here the way
loss_restatement.cauchy_bounds builds its own, from the measured error of the device library's log1p and log.  Also the same
quantities in 60-digit decimal arithmetic, which the bounds are checked against.  Test infrastructure, not part of the
product."""
import decimal

import numpy as np

import loss_restatement as LR

U = 2.0 ** -52                                  # one ulp, relative
U0 = 2.0 ** -53                                 # one rounding
SWITCH = 2.0 ** -6                              # |e| up to here: the series
MU_FLOOR = 2.0 ** -20                           # the default floor of nonlin_amd.Poisson
U_LOG1P = LR.U_LOG1P
# Error of the device library's log in ulp over [1e-12, 0.5] (the arguments u of the e < -0.5 branch), rounded up to an
# integer: the ceiling of the maximum tests/test_gpu_pois.py::test_log_accuracy measures, by the rule of U_LOG1P.
U_LOG = 1
BRANCHES = ("masked", "y0", "series", "log1p", "log", "floor")


def apply(y, w, f, r, log1p=np.log1p, log=np.log):
    """(out, g, D, branch) of the inner residuals r = model - y for counts y, mask w (None: none) and floor f, by the header's
    table; branch: the index in BRANCHES of the path a row takes (floor rows: the path of their base point; -1: NaN rows),
    and low, the rows below the floor, is branch's companion in branches().  log1p / log: the library functions (the
    perturbation study passes its own)."""
    return _apply(y, w, f, r, log1p, log)[:4]


def branches(y, w, f, r):
    """(branch, low) of every row."""
    v = _apply(y, w, f, r, np.log1p, np.log)
    return v[3], v[4]


def _apply(y, w, f, r, log1p, log):
    r = np.asarray(r, dtype=np.float64)
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), r.shape)
    nan = np.float64("nan")
    if not (f > 0.0 and np.isfinite(f)):
        bad = np.full(r.shape, nan)
        return bad, bad.copy(), bad.copy(), np.full(r.shape, -1), np.zeros(r.shape, bool)
    has_w = w is not None
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), r.shape) if has_w else np.ones(r.shape)
    masked = (wv == 0.0) if has_w else np.zeros(r.shape, bool)
    isnan = ~masked & ((has_w & (wv != 1.0)) | ~(y >= 0.0) | ~np.isfinite(y))
    with np.errstate(all="ignore"):
        mu = r + y
        low = mu < f
        rr = np.where(low, f - y, r)
        # y == 0
        D0 = 2.0 * rr
        s0 = np.sqrt(D0)
        g0 = 1.0 / s0
        # y > 0
        e = rr / y
        a = np.fabs(e)
        t = rr + y
        u = t / y
        q = np.full(r.shape, 1.0 / 13)
        for k in range(12, 1, -1):
            q = e * q
            q = 1.0 / k - q
        z = e * e
        hs = z * q
        ser = a <= SWITCH
        far = e < -0.5
        safe_u = np.where(far & (y > 0.0) & ~ser, u, 1.0)
        safe_e = np.where(~far & (y > 0.0) & ~ser, e, 0.0)
        l = np.where(far, log(safe_u), log1p(safe_e))
        l = np.where(np.isnan(e), nan, l)
        hd = e - l
        h = np.where(ser, hs, hd)
        D = 2.0 * y
        D = D * h
        s = np.sqrt(D)
        d = np.copysign(s, e)
        us = u * s
        g = np.where(e == 0.0, 1.0 / np.sqrt(y), a / us)
        zero = y == 0.0
        d = np.where(zero, s0, d)
        g = np.where(zero, g0, g)
        D = np.where(zero, D0, D)
        v = mu - f
        v = g * v
        out = np.where(low, d + v, d)
    branch = np.where(zero, 1, np.where(ser, 2, np.where(far, 4, 3)))
    branch = np.where(masked, 0, np.where(isnan | np.isnan(r), -1, branch))
    out = np.where(masked, 0.0, np.where(isnan, nan, out))
    g = np.where(masked, 0.0, np.where(isnan, nan, g))
    D = np.where(masked, 0.0, np.where(isnan, nan, D))
    return out, g, D, branch, low & ~masked & ~isnan


def residual(y, w, f, r, **kw):
    return apply(y, w, f, r, **kw)[0]


def jacobian(y, w, f, r, J, **kw):
    """J' (m, n) = g_i * J[i][j], g from the inner residual r (m) at the same point; a masked row is +0.0 whatever J holds."""
    out, g, D, br = apply(y, w, f, r, **kw)
    return np.where((br == 0)[:, None], 0.0, g[:, None] * np.asarray(J))


def uses_library(branch):
    """Rows whose value carries log1p or log."""
    return (branch == 3) | (branch == 4)


# ------------------------------------------------------------------------------------------------ exact arithmetic
def exact(y, rr, prec=60):
    """(d, g) of the table above the floor for ONE row in `prec`-digit decimal arithmetic: d = sign(e) sqrt(2 (rr - y log(1 +
    rr / y))) and g = (1 - y / mu) / d, mu = rr + y; y = 0: d = sqrt(2 rr), g = 1 / d; rr = 0: d = 0, g = 1 / sqrt(y)."""
    with decimal.localcontext() as c:
        c.prec = prec
        Y, R = decimal.Decimal(float(y)), decimal.Decimal(float(rr))
        if Y == 0:
            d = (2 * R).sqrt()
            return d, 1 / d
        if R == 0:
            return decimal.Decimal(0), 1 / Y.sqrt()
        mu = R + Y
        D = 2 * (R - Y * (mu / Y).ln())
        d = D.sqrt().copy_sign(R)
        return d, (1 - Y / mu) / d


def rel_err(got, want):
    """|got - want| / |want| of a float against a Decimal, as a float."""
    with decimal.localcontext() as c:
        c.prec = 60
        return float(abs(decimal.Decimal(float(got)) - want) / abs(want))


# ------------------------------------------------------------------------------------------------ bounds
def _kappa(e, h):
    """|e h'(e) / h|, h = e - log(1 + e): what a relative error of e costs h when every use of e moves together."""
    return e * e / ((1.0 + e) * h)


def exact_bounds(y, rr, ufn=None):
    """First-order RELATIVE bounds of d and g of rows above the floor against exact arithmetic, derived from the stated
    operations: every operation adds a rounding U0; a library function adds ufn ulp of its result (default: U_LOG1P for
    log1p, U_LOG for log).
      e = rr / y                 U0;   u = (rr + y) / y    2 U0, or U0 where e < -0.5 (rr + y is then exact: Sterbenz)
      series                     q: the last Horner step subtracts from the exact constant 1/2, U0 |q| <= 0.505 U0, and takes
                                 SWITCH times what the step before carries (its constant, its subtraction, the product: below
                                 1.04 U0): 0.521 U0 of a q >= 0.4948, below 1.1 U0; z = e*e: U0; h = z*q: U0; the truncation,
                                 e^12 * 2/14, is below 2^-74; e's own error, moving every use of e together, costs kappa U0
      log1p branch               e's error moves e and log1p(e) together: kappa U0; the function's error is ufn U |l| / h;
                                 the subtraction U0
      log branch                 |e| U0 / h for e, eps_u / h for the argument, ufn U |l| / h, the subtraction U0
      D = (2 y) h                U0 (2 y is exact);   s = sqrt(D): half of D's, plus U0;   d = copysign(s, e): s's
      g = a / (u s)              a: U0, u: eps_u, the product U0, s: its own, the quotient U0
      y == 0                     d = sqrt(2 rr): U0;  g = 1 / d: 2 U0          e == 0: d exact, g = 1 / sqrt(y): 2 U0"""
    y = np.asarray(y, dtype=np.float64)
    rr = np.broadcast_to(np.asarray(rr, dtype=np.float64), y.shape)
    ul1, ul = (U_LOG1P, U_LOG) if ufn is None else (ufn, ufn)
    with np.errstate(all="ignore"):
        ys = np.where(y > 0.0, y, 1.0)
        e = np.where(y > 0.0, rr / ys, 1.0)
        a = np.fabs(e)
        ser = a <= SWITCH
        far = e < -0.5
        eu = np.where(far, U0, 2 * U0)
        el = e.astype(np.longdouble)
        l = np.where(far, np.log(np.where(far, 1.0 + el, 1.0)), np.log1p(np.where(far, 0.0, el)))
        h = np.where(ser, el * el / 2, el - l).astype(np.float64)
        h = np.where(h > 0.0, h, 1.0)
        l = np.abs(l).astype(np.float64)
        kap = np.where(ser, 2.0 / ((1.0 + e) * (1.0 - SWITCH)), _kappa(e, h))
        bh = np.where(ser, kap * U0 + 1.1 * U0 + U0 + U0 + 2.0 ** -74,
                      np.where(far, (a * U0 + eu + ul * U * l) / h + U0, kap * U0 + ul1 * U * l / h + U0))
        bs = 0.5 * (bh + U0) + U0
        bg = U0 + eu + U0 + bs + U0
        zero_y, zero_e = y == 0.0, (y > 0.0) & (rr == 0.0)
        bd = np.where(zero_y, U0, np.where(zero_e, 0.0, bs))
        bg = np.where(zero_y | zero_e, 2 * U0, bg)
    return bd, bg


def device_bounds(y, w, f, r):
    """First-order ABSOLUTE bounds of |device - numpy| for out and g of every row (0.0 where the row reaches no library
    function: bit for bit), as loss_restatement.cauchy_bounds carries them: l differs by (ufn + 1) ulp of l -- the device
    function's error and 1 ulp for numpy's --; h = e - l adds a rounding of h; D = (2 y) h one of D; the exact sqrt halves that and
    adds a rounding of s; g = a / (u s), a and u carrying no error, takes s's relative error and adds the roundings of the
    product and of the quotient.  Below the floor out = d + g v: d's and g's differences, a rounding of the product and one of
    the sum."""
    out, g, D, br, low = _apply(y, w, f, r, np.log1p, np.log)
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), out.shape)
    r = np.asarray(r, dtype=np.float64)
    lib = uses_library(br)
    with np.errstate(all="ignore"):
        rr = np.where(low, f - y, r)
        ys = np.where(lib, y, 1.0)
        e = np.where(lib, rr / ys, 1.0)
        far = e < -0.5
        l = np.where(far, np.log(np.where(far, (rr + ys) / ys, 1.0)), np.log1p(np.where(far, 0.0, e)))
        h = np.where(lib, e - l, 1.0)
        ufn = np.where(far, U_LOG, U_LOG1P) + 1.0
        bh = ufn * U * np.abs(l) / np.abs(h) + U
        bs = 0.5 * (bh + U) + U
        bg_rel = bs + 2 * U
        d = np.where(lib, np.copysign(np.sqrt((2.0 * ys) * h), e), 0.0)
        bd = bs * np.abs(d)
        bg = bg_rel * np.abs(g)
        v = np.where(low, (r + y) - f, 0.0)
        bo = np.where(low, bd + bg * np.abs(v) + U * np.abs(g * v) + U * np.abs(out), bd)
    return np.where(lib, bo, 0.0), np.where(lib, bg, 0.0)
