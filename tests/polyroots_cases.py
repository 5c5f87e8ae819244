"""The fixed, seeded families of polynomials the root-finder tests run (tests/test_polyroots_cpu.py,
tests/test_gpu_polyroots.py, tests/golden/make_poly_roots_study.py).  numpy only.  Every case is a float64 coefficient
vector, constant first (c(1) + c(2) x + ...), as polynomial%initialize takes it.

  a  the reference's own vectors: x^3 - 4x^2 + x + 6 (tests/nonlin_test_poly.f90:53-84) and the roots example's
     x^3 - 2x - 1
  b  standard normal coefficients: orders 1, 2, 3, 5, 8, 9, 16 fifty each; orders 33, 64, 100 six each
  c  built from prescribed roots, orders 4..20, three kinds each: real roots in [-2, 2]; complex pairs in the disc of
     radius 1.5 (and one real root when the order is odd); pairs on the unit circle (and the root 1 when odd)
  d  badly scaled: a_k 10^(+k) and a_k 10^(-k), a_k standard normal, orders 6 and 12, ten each
  e  structure: zero constant coefficient(s); the double root (x - 1)^2 (x + 2); Wilkinson 10 and 15; x^n - 1, n = 7, 64
  f  failure rows: leading coefficient 0; a NaN coefficient; an infinite coefficient
"""
import numpy as np

SEED = 20261016

ZERO_CASES = [([0.0, 0.0, 1.0, 2.0, 3.0], 2), ([0.0, -6.0, 1.0, 4.0, 1.0], 1), ([0.0, 0.0, 0.0, 1.0, -3.0, 2.0], 3)]


def _from_roots(roots):
    """Coefficients (constant first) of prod (x - r), accumulated in complex128; the imaginary parts cancel to rounding."""
    c = np.array([1.0 + 0.0j])
    for r in roots:
        c = np.convolve(c, np.array([-r, 1.0]))
    return np.ascontiguousarray(c.real)


def family_a():
    return [np.array([6.0, 1.0, -4.0, 1.0]), np.array([-1.0, -2.0, 0.0, 1.0])]


def family_b():
    rng = np.random.default_rng(SEED + 1)
    out = []
    for order in (1, 2, 3, 5, 8, 9, 16):
        out += [rng.standard_normal(order + 1) for _ in range(50)]
    for order in (33, 64, 100):
        out += [rng.standard_normal(order + 1) for _ in range(6)]
    return out


def family_c():
    rng = np.random.default_rng(SEED + 2)
    out = []
    for order in range(4, 21):
        out.append(_from_roots(list(rng.uniform(-2.0, 2.0, order))))
        roots = []
        for _ in range(order // 2):
            z = 1.5 * np.sqrt(rng.uniform()) * np.exp(1j * rng.uniform(0.1, np.pi - 0.1))
            roots += [z, np.conj(z)]
        if order % 2:
            roots.append(rng.uniform(-1.5, 1.5))
        out.append(_from_roots(roots))
        roots = []
        for _ in range(order // 2):
            z = np.exp(1j * rng.uniform(0.1, np.pi - 0.1))
            roots += [z, np.conj(z)]
        if order % 2:
            roots.append(1.0)
        out.append(_from_roots(roots))
    return out


def family_d():
    rng = np.random.default_rng(SEED + 3)
    out = []
    for order in (6, 12):
        for sgn in (1.0, -1.0):
            for _ in range(10):
                a = rng.standard_normal(order + 1)
                out.append(a * 10.0 ** (sgn * np.arange(order + 1)))
    return out


def family_e():
    out = [np.array(c) for c, _ in ZERO_CASES]
    out.append(np.array([2.0, -3.0, 0.0, 1.0]))                     # (x - 1)^2 (x + 2)
    for n in (10, 15):
        out.append(_from_roots([float(k) for k in range(1, n + 1)]))   # Wilkinson (exact in float64 at these orders)
    for n in (7, 64):
        c = np.zeros(n + 1)
        c[0] = -1.0
        c[n] = 1.0
        out.append(c)
    return out


def family_f():
    """(coefficients, expected info)."""
    return [(np.array([1.0, 2.0, 3.0, 0.0]), 210), (np.array([1.0, np.nan, 3.0, 1.0]), 201),
            (np.array([1.0, 2.0, np.inf, 1.0]), 201), (np.array([1.0, 2.0, -3.0, 0.0, 1.0, 0.0]), 210),
            (np.array([np.nan, 2.0, -3.0, 0.0, 1.0, 2.0]), 201)]


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}


def companion(c):
    """The companion matrix exactly as src/nonlin_polynomials.f90:346-353."""
    n = len(c) - 1
    m = np.zeros((n, n))
    for i in range(n):
        m[i, n - 1] = -c[i] / c[n]
        if i < n - 1:
            m[i + 1, i] = 1.0
    return m


def by_order(cases):
    """{order: [coefficient vectors]} in first-seen order."""
    out = {}
    for c in cases:
        out.setdefault(len(c) - 1, []).append(c)
    return out
