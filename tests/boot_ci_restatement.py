"""The studentised and the BCa interval of the bootstrap (include/nonlin_hip_boot_ci.h: nlh_boot_student_batch,
nlh_boot_jackknife_batch, nlh_boot_accel_batch, nlh_boot_bca_batch, nlh_boot_bca_levels), restated in numpy on
tests/boot_restatement.py's sort, quantile and sum: every floating-point step one IEEE operation in the header's order.  What
goes through a library function -- ppnd16's tails (log), alpha (erfc) -- is Python's math module here.  Test infrastructure,
not part of the product."""
import math

import numpy as np

from boot_restatement import stable_sort, quantile, tree_sum

DEGENERATE, NO_ACCEL, BAD_DENOM, NO_REPLICA = 1, 2, 4, 8
# Wichura, AS 241, PPND16: the header's coefficients, highest first
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _horner(c, r):
    s = c[0]
    for k in c[1:]:
        s = s * r + k
    return s


def central(p):
    """Does ppnd16(p) stay in the branch that reaches no library function."""
    return abs(p - 0.5) <= 0.425


def ppnd16(p):
    """z with Phi(z) = p for 0 < p < 1 (Python floats: one IEEE operation per step)."""
    p = float(p)
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return (_horner(_A, r) * q) / _horner(_B, r)
    r = p if q <= 0.0 else 1.0 - p
    r = math.sqrt(-math.log(r))
    if r <= 5.0:
        r = r - 1.6
        z = _horner(_C, r) / _horner(_D, r)
    else:
        r = r - 5.0
        z = _horner(_E, r) / _horner(_F, r)
    return -z if q < 0.0 else z


def levels(level):
    qlo = (1.0 - float(level)) / 2.0
    return qlo, 1.0 - qlo


def bca_levels(c2, cnt, a, level):
    """(z0, alpha_lo, alpha_hi, flag, u): nlh_boot_bca_levels; u (None where it is not formed) for the tests."""
    qlo, qhi = levels(level)
    if cnt == 0:
        return math.nan, math.nan, math.nan, NO_REPLICA, None
    flag = 0
    if not math.isfinite(a):
        flag |= NO_ACCEL
        a = 0.0
    if c2 == 0 or c2 == 2 * cnt:
        return (-math.inf if c2 == 0 else math.inf), qlo, qhi, flag | DEGENERATE, None
    u = float(c2) / float(2 * cnt)
    z0 = ppnd16(u)
    alpha = [qlo, qhi]
    for t, z in enumerate((ppnd16(qlo), ppnd16(qhi))):
        s = z0 + z
        den = 1.0 - a * s
        if not den > 0.0:
            flag |= BAD_DENOM
            continue
        w = z0 + s / den
        alpha[t] = 0.5 * math.erfc(-(w * 0.70710678118654752))
    return z0, alpha[0], alpha[1], flag, u


def student(xs, sigs, x, sigma, level):
    """(lo, hi [nprob, n], nvalid_t [nprob, n]): nlh_boot_student_batch."""
    xs, sigs = np.asarray(xs, dtype=np.float64), np.asarray(sigs, dtype=np.float64)
    nrep, nprob, n = xs.shape
    qlo, qhi = levels(level)
    lo, hi = np.full((nprob, n), np.nan), np.full((nprob, n), np.nan)
    nvalid_t = np.zeros((nprob, n), dtype=np.int32)
    rows = np.isfinite(xs).all(axis=2)
    with np.errstate(all="ignore"):
        for p in range(nprob):
            for j in range(n):
                ok = rows[:, p] & np.isfinite(sigs[:, p, j]) & (sigs[:, p, j] > 0.0)
                cnt = int(ok.sum())
                nvalid_t[p, j] = cnt
                xh, sg = x[p, j], sigma[p, j]
                if cnt == 0 or not np.isfinite(xh) or not (np.isfinite(sg) and sg > 0.0):
                    continue
                t = stable_sort((xs[ok, p, j] - xh) / sigs[ok, p, j])
                tlo, thi = quantile(t, qlo), quantile(t, qhi)
                lo[p, j] = xh - thi * sg
                hi[p, j] = xh - tlo * sg
    return lo, hi, nvalid_t


def jackknife(w, nprob, m, row0=0, nrows=None):
    """wout [nrows, nprob, m]: nlh_boot_jackknife_batch."""
    nrows = m - row0 if nrows is None else nrows
    base = np.ones((nprob, m)) if w is None else np.asarray(w, dtype=np.float64)
    out = np.broadcast_to(base, (nrows, nprob, m)).copy()
    for r in range(nrows):
        out[r, :, row0 + r] = 0.0
    return out


def _masked_tree_sum(v, ok):
    """The 64-partial sum and tree of v[i] over the i with ok[i], partial i mod 64 (the ROW's number), ascending i: tree_sum
    itself where every row counts."""
    if ok.all():
        return tree_sum(v)
    part = np.zeros(64)
    with np.errstate(all="ignore"):
        for i0 in range(0, len(v), 64):
            idx = np.flatnonzero(ok[i0:i0 + 64])
            part[idx] = part[idx] + v[i0 + idx]
        off = 32
        while off:
            part[:off] = part[:off] + part[off:2 * off]
            off //= 2
    return part[0]


def accel(xjack, w=None):
    """(a [nprob, n], njack [nprob]): nlh_boot_accel_batch."""
    xjack = np.asarray(xjack, dtype=np.float64)
    m, nprob, n = xjack.shape
    a = np.zeros((nprob, n))
    njack = np.zeros(nprob, dtype=np.int32)
    for p in range(nprob):
        ok = np.isfinite(xjack[:, p, :]).all(axis=1)
        if w is not None:
            ok &= np.asarray(w)[p] != 0.0
        c = int(ok.sum())
        njack[p] = c
        if c < 2:
            continue
        for j in range(n):
            v = np.where(ok, xjack[:, p, j], 0.0)
            with np.errstate(all="ignore"):
                mean = _masked_tree_sum(v, ok) / np.float64(c)
                d = mean - v
                dd = d * d
                s2, s3 = _masked_tree_sum(dd, ok), _masked_tree_sum(dd * d, ok)
                if s2 != 0.0:
                    val = s3 / (6.0 * (s2 * np.sqrt(s2)))
                    a[p, j] = val if np.isfinite(val) else 0.0
    return a, njack


def bca_counts(xs, x):
    """(c2 [nprob, n], cnt [nprob]) of `bca`: the integers."""
    xs = np.asarray(xs, dtype=np.float64)
    rows = np.isfinite(xs).all(axis=2)
    cnt = rows.sum(axis=0).astype(np.int32)
    nrep, nprob, n = xs.shape
    c2 = np.zeros((nprob, n), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(nprob):
            v = xs[rows[:, p], p, :]
            c2[p] = 2 * (v < x[p][None, :]).sum(axis=0) + (v == x[p][None, :]).sum(axis=0)
    return c2, cnt


def bca(xs, x, a, level, alphas=None):
    """(lo, hi, z0, alpha_lo, alpha_hi [nprob, n], flags [nprob, n], nvalid [nprob]): nlh_boot_bca_batch.  alphas = (alpha_lo,
    alpha_hi) arrays: the quantiles are taken at THESE levels instead of the restatement's own (lo and hi are exact given
    the alphas that come back with them)."""
    xs = np.asarray(xs, dtype=np.float64)
    nrep, nprob, n = xs.shape
    rows = np.isfinite(xs).all(axis=2)
    c2, cnt = bca_counts(xs, x)
    out = [np.full((nprob, n), np.nan) for _ in range(5)]
    flags = np.zeros((nprob, n), dtype=np.int32)
    for p in range(nprob):
        for j in range(n):
            if cnt[p] == 0 or not np.isfinite(x[p, j]):
                flags[p, j] = NO_REPLICA
                continue
            z0, alo, ahi, flag, _ = bca_levels(int(c2[p, j]), int(cnt[p]), float(a[p, j]), level)
            flags[p, j] = flag
            v = stable_sort(xs[rows[:, p], p, j])
            qa, qb = (alo, ahi) if alphas is None else (alphas[0][p, j], alphas[1][p, j])
            out[0][p, j], out[1][p, j] = quantile(v, qa), quantile(v, qb)
            out[2][p, j], out[3][p, j], out[4][p, j] = z0, alo, ahi
    return tuple(out) + (flags, cnt)
