"""What tests/test_polyroots_cpu.py and tests/golden/make_poly_roots_study.py measure on the families of
tests/polyroots_cases.py: the backward-error-style ratio r(z) = |p(z)| / sum_k |a_k| |z|^k of a computed root, in mpmath at
60 digits, for the restatement's roots and for LAPACK's (numpy.linalg.eigvals on the companion matrix, which is what the
reference calls), the one-to-one matching of the two root sets, and the forward error against mpmath.polyroots.  CPU-side
test infrastructure (mpmath, scipy); the GPU tests do not import it."""
import mpmath
import numpy as np
from scipy.optimize import linear_sum_assignment

import polyroots_cases as cases
import polyroots_restatement as rs

EPS = 2.22e-16
mpmath.mp.dps = 60


def ratio_r(c, z):
    """r(z) for the float64 coefficients c (constant first); 0 where z == 0 and a_0 == 0 (a root that is exactly right)."""
    if z == 0 and c[0] == 0.0:
        return 0.0
    zm = mpmath.mpc(z.real, z.imag)
    az = abs(zm)
    p = mpmath.mpc(0)
    s = mpmath.mpf(0)
    for k in range(len(c) - 1, -1, -1):
        p = p * zm + mpmath.mpf(float(c[k]))
        s = s * az + abs(mpmath.mpf(float(c[k])))
    return float(abs(p) / s)


def ours(c, stats=None):
    z, info = rs.poly_roots([float(v) for v in c], stats=stats)
    return np.array([complex(re, im) for re, im in z]), info


def lapack(c):
    return np.linalg.eigvals(cases.companion(c))


def match(z, w):
    """Minimum-cost one-to-one assignment of z to w; returns the permutation p with z[i] <-> w[p[i]]."""
    assert len(z) == len(w)
    cost = np.abs(np.asarray(z)[:, None] - np.asarray(w)[None, :])
    rows, cols = linear_sum_assignment(cost)
    assert list(rows) == list(range(len(z)))
    return cols


def true_roots(c):
    """mpmath.polyroots of the float64 coefficients, 60 digits."""
    coeffs = [mpmath.mpf(float(v)) for v in c[::-1]]
    r = mpmath.polyroots(coeffs, maxsteps=2000, extraprec=2000)
    return r


def forward_error(z, truth):
    """max over the matched pairs of |z - t| / max(1, |t|), the differences taken in mpmath."""
    t64 = np.array([complex(t) for t in truth])
    p = match(z, t64)
    worst = 0.0
    for i, zz in enumerate(z):
        t = truth[p[i]]
        e = abs(mpmath.mpc(zz.real, zz.imag) - t) / max(mpmath.mpf(1), abs(t))
        worst = max(worst, float(e))
    return worst


def measure_family(name, forward=False):
    """{"max_r_lapack", "max_r_ours", "ratio"} and, forward, the same three for the forward error."""
    mo = ml = fo = fl = 0.0
    for c in cases.FAMILIES[name]():
        z, info = ours(c)
        assert info == 0
        w = lapack(c)
        match(z, w)
        mo = max(mo, max(ratio_r(c, v) for v in z))
        ml = max(ml, max(ratio_r(c, v) for v in w))
        if forward:
            t = true_roots(c)
            fo = max(fo, forward_error(z, t))
            fl = max(fl, forward_error(w, t))
    out = {"max_r_lapack": ml, "max_r_ours": mo, "ratio": mo / max(ml, EPS)}
    if forward:
        out.update({"max_fwd_lapack": fl, "max_fwd_ours": fo, "fwd_ratio": fo / max(fl, EPS)})
    return out


def bound_from_study(study):
    """M: the smallest power of two that is at least twice the largest measured family ratio, never above 16."""
    worst = max(v["ratio"] for v in study["families"].values())
    m = 1
    while m < 2.0 * worst:
        m *= 2
    return min(m, 16)
